"""gfx950 buffer kernels (fill / verify / reduce / diagnose / checked copy) on torch tensors,
plus the plain-PyTorch reference implementations they are tested against."""

from .buffers import (  # noqa: F401
    CopyCheck,
    Extent,
    GranuleRecord,
    VerifyResult,
    checksum,
    copy_checked_,
    diagnose,
    diagnose_records,
    fill_,
    reference_bytes,
    reference_copy_check,
    reference_diagnose,
    reference_verify,
    reference_words,
    verify,
)
