"""gfx950 buffer kernels (fill / verify / reduce / diagnose) on torch tensors,
plus the plain-PyTorch reference implementations they are tested against."""

from .buffers import (  # noqa: F401
    Extent,
    GranuleRecord,
    VerifyResult,
    checksum,
    diagnose,
    diagnose_records,
    fill_,
    reference_bytes,
    reference_diagnose,
    reference_verify,
    reference_words,
    verify,
)
