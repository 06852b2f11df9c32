// Host-only unit tests (tier T0 in SURVEY.md §4): no GPU, no MPI launcher.
// Built with g++ by `make host`; run directly or through tests/test_host_unit.py.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "app.hpp"
#include "block_split.hpp"
#include "bootstrap.hpp"
#include "common.hpp"
#include "ipc_blocks.hpp"
#include "prng.hpp"
#include "push_plan.hpp"
#include "rccl_log.hpp"
#include "report.hpp"
#include "routing.hpp"
#include "runner.hpp"
#include "schedule.hpp"
#include "stats.hpp"
#include "stream_layout.hpp"
#include "stream_plan.hpp"
#include "transport.hpp"
#include "units.hpp"

using namespace p2p;

static std::atomic<int> g_failures{0};
static std::atomic<int> g_checks{0};

#define EXPECT(cond)                                                       \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      ++g_failures;                                                        \
      std::fprintf(stderr, "  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

#define EXPECT_NEAR(a, b, tol) EXPECT(std::fabs((a) - (b)) <= (tol))

struct TestCase {
  const char* name;
  std::function<void()> fn;
};
static std::vector<TestCase>& registry() {
  static std::vector<TestCase> r;
  return r;
}
#define TEST(name)                                              \
  static void name();                                           \
  static bool name##_reg = (registry().push_back({#name, name}), true); \
  static void name()

// --------------------------------------------------------------- units ----

TEST(test_parse_size) {
  EXPECT(parse_size("4096") == 4096);
  EXPECT(parse_size("4K") == 4096);
  EXPECT(parse_size("4KiB") == 4096);
  EXPECT(parse_size("32M") == 32u << 20);
  EXPECT(parse_size("32mb") == 32u << 20);
  EXPECT(parse_size("1G") == 1ull << 30);
  EXPECT(parse_size("4G") == 4ull << 30);  // > INT_MAX: the reference's int msg_size could not
  EXPECT(parse_size("1.5K") == 1536);
  EXPECT(format_size(32u << 20) == "32M");
  EXPECT(format_size(4096) == "4K");
  EXPECT(format_size(1000) == "1000");
  EXPECT(format_size(4ull << 30) == "4G");
}

TEST(test_parse_size_list) {
  auto v = parse_size_list("4K:64K");
  EXPECT(v.size() == 5);
  EXPECT(v.front() == 4096 && v.back() == 65536);
  auto w = parse_size_list("4K:1M:4");
  EXPECT(w.size() == 5);  // 4K 16K 64K 256K 1M
  EXPECT(w.back() == 1u << 20);
  auto x = parse_size_list("4K,1M,3M");
  EXPECT(x.size() == 3 && x[2] == 3u << 20);
  auto big = parse_size_list("4K:4G");
  EXPECT(big.size() == 21);
}

TEST(test_gbps_units) {
  // Reference: throughput = msg_size * 8. / time / 1e9 (p2p_matrix.cc:177)
  EXPECT_NEAR(gbps(33554432.0, 1e-3), 268.435456, 1e-9);
  EXPECT_NEAR(gbytes_per_s(33554432.0, 1e-3), 33.554432, 1e-12);
}

// --------------------------------------------------------- block split ----

// split_blocks against its rule, written out: need = max(1, ceil(nvec /
// block_vecs)); every job gets its need while the needs fit the cap, else
// max(1, need * cap / total), never more than its need; block_begin holds the
// prefix sums.
static void expect_split(const std::vector<uint64_t>& nvec, uint64_t block_vecs, uint64_t cap) {
  const int cnt = static_cast<int>(nvec.size());
  std::vector<uint32_t> begin(nvec.size() + 1, 0xDEADu);
  const uint32_t grid = split_blocks(nvec.data(), cnt, block_vecs, cap, begin.data());
  std::vector<uint64_t> need(nvec.size());
  uint64_t total = 0;
  for (int i = 0; i < cnt; ++i) total += need[i] = std::max<uint64_t>(1, (nvec[i] + block_vecs - 1) / block_vecs);
  uint64_t sum = 0;
  for (int i = 0; i < cnt; ++i) {
    EXPECT(begin[i] == sum);
    EXPECT(begin[i + 1] >= begin[i]);
    const uint64_t share = begin[i + 1] - begin[i];
    EXPECT(share >= 1 && share <= need[i]);
    if (total <= cap)
      EXPECT(share == need[i]);
    else
      EXPECT(share == std::max<uint64_t>(1, need[i] * cap / total));
    sum += share;
  }
  EXPECT(begin[cnt] == sum && grid == sum);
}

TEST(test_split_blocks) {
  // One job: under the cap (its need, 3 blocks of 256 vectors), and over it.
  expect_split({600}, 256, 1u << 20);
  expect_split({600}, 256, 2);
  // 32 equal jobs: equal shares (what plan_copy_group's `uniform` detects),
  // under the cap and over it.
  for (uint64_t cap : {uint64_t{1} << 20, uint64_t{4096}, uint64_t{40}}) {
    std::vector<uint64_t> equal(32, (32u << 20) / 16);
    expect_split(equal, 256, cap);
    uint32_t begin[33];
    split_blocks(equal.data(), 32, 256, cap, begin);
    for (int i = 1; i < 32; ++i) EXPECT(begin[i + 1] - begin[i] == begin[1] - begin[0]);
  }
  // One huge job beside 31 one-block jobs under a small cap: the small ones
  // keep their one block, the huge one is cut down.
  std::vector<uint64_t> mixed(32, 100);
  mixed[7] = (uint64_t{4} << 30) / 16;
  expect_split(mixed, 256, 64);
  expect_split(mixed, 2048, 4096);  // the batched verify's 32 KiB chunks, 16 workgroups x 256 CUs
  // A zero-byte job needs one workgroup, alone and among others.
  expect_split({0}, 256, 1u << 20);
  expect_split({0, 4096, 0, 1}, 256, 1u << 20);
  expect_split({0, 1u << 20, 0}, 256, 3);
  uint32_t begin[2];
  EXPECT(split_blocks(std::vector<uint64_t>{0}.data(), 1, 2048, 16, begin) == 1 && begin[0] == 0 && begin[1] == 1);
}

// --------------------------------------------------------------- stats ----

TEST(test_stats) {
  std::vector<double> s{5, 1, 4, 2, 3};
  EXPECT_NEAR(percentile(s, 50), 3.0, 1e-12);
  EXPECT_NEAR(percentile(s, 0), 1.0, 1e-12);
  EXPECT_NEAR(percentile(s, 100), 5.0, 1e-12);
  EXPECT_NEAR(percentile({1, 2, 3, 4}, 50), 2.5, 1e-12);
  EXPECT_NEAR(percentile({1, 2, 3, 4}, 90), 3.7, 1e-12);
  Summary m = summarize(s);
  EXPECT(m.n == 5);
  EXPECT_NEAR(m.mean, 3.0, 1e-12);
  EXPECT_NEAR(m.stdev, std::sqrt(2.5), 1e-12);
  EXPECT(summarize({}).n == 0);
  std::vector<double> mat{0, 10, 20, 30, 0, 40, 50, 60, 0};
  MatrixSummary ms = summarize_offdiag(mat, 3);
  EXPECT(ms.cells == 6);
  EXPECT_NEAR(ms.min, 10, 1e-12);
  EXPECT_NEAR(ms.mean, 35, 1e-12);
  EXPECT_NEAR(ms.max, 60, 1e-12);
}

// ------------------------------------------------------------ schedules ----

static std::multiset<std::pair<int, int>> all_flows(const Schedule& s) {
  std::multiset<std::pair<int, int>> m;
  for (const auto& p : s.phases)
    for (const auto& f : p.flows) m.insert({f.src, f.dst});
  return m;
}

TEST(test_schedules_valid) {
  for (int n = 1; n <= 9; ++n) {
    for (Mode m : {Mode::Pair, Mode::Ring, Mode::AllPairs, Mode::Tournament, Mode::Self})
      for (Direction d : {Direction::Uni, Direction::Bi}) {
        Schedule s = make_schedule(m, d, n);
        EXPECT(validate(s).empty());
        EXPECT(s.nranks == n);
      }
  }
}

TEST(test_pair_schedule_reference_order) {
  // p2p_matrix.cc:141-145: for src { for dst { barrier; ... } }, diagonal idle.
  Schedule s = make_pair_schedule(3, Direction::Uni);
  EXPECT(s.phases.size() == 9);
  int k = 0;
  for (int src = 0; src < 3; ++src)
    for (int dst = 0; dst < 3; ++dst, ++k) {
      const Phase& p = s.phases[k];
      EXPECT(p.row == src && p.col == dst);
      EXPECT(p.idle == (src == dst));
      if (src != dst) {
        EXPECT(p.flows.size() == 1);
        EXPECT(p.ranks[src].send_to == std::vector<int>{dst});
        EXPECT(p.ranks[dst].recv_from == std::vector<int>{src});
        for (int r = 0; r < 3; ++r)
          if (r != src && r != dst) EXPECT(!p.participates(r));
      }
    }
  Schedule b = make_pair_schedule(2, Direction::Bi);
  EXPECT(b.phases[1].flows.size() == 2);  // both endpoints send and receive (:211-249)
  EXPECT(b.phases[1].ranks[0].send_to == std::vector<int>{1});
  EXPECT(b.phases[1].ranks[0].recv_from == std::vector<int>{1});
}

TEST(test_round_robin_rounds) {
  for (int n = 2; n <= 12; ++n) {
    auto rounds = round_robin_rounds(n);
    EXPECT(static_cast<int>(rounds.size()) == (n % 2 == 0 ? n - 1 : n));
    std::set<std::pair<int, int>> seen;
    for (auto& r : rounds) {
      std::set<int> busy;
      for (auto& pr : r) {
        EXPECT(pr.first < pr.second);
        EXPECT(busy.insert(pr.first).second);  // disjoint within a round
        EXPECT(busy.insert(pr.second).second);
        EXPECT(seen.insert(pr).second);        // each pair once overall
      }
      EXPECT(static_cast<int>(r.size()) == n / 2);
    }
    EXPECT(static_cast<int>(seen.size()) == n * (n - 1) / 2);
  }
}

TEST(test_tournament_covers_matrix) {
  for (int n = 2; n <= 9; ++n) {
    std::multiset<std::pair<int, int>> want;
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < n; ++b)
        if (a != b) want.insert({a, b});
    EXPECT(all_flows(make_tournament_schedule(n, Direction::Uni)) == want);
    EXPECT(all_flows(make_tournament_schedule(n, Direction::Bi)) == want);
    // Uni: no rank is both sender and receiver in one phase -> one link per pair.
    for (const auto& p : make_tournament_schedule(n, Direction::Uni).phases)
      for (const auto& ro : p.ranks) EXPECT(ro.send_to.size() + ro.recv_from.size() <= 1);
  }
}

TEST(test_ring_and_allpairs) {
  Schedule r = make_ring_schedule(4, Direction::Uni);
  EXPECT(r.phases.size() == 1);
  std::multiset<std::pair<int, int>> ring{{0, 1}, {1, 2}, {2, 3}, {3, 0}};
  EXPECT(all_flows(r) == ring);
  Schedule rb = make_ring_schedule(4, Direction::Bi);
  EXPECT(rb.phases[0].flows.size() == 8);
  Schedule r2 = make_ring_schedule(2, Direction::Bi);
  EXPECT(r2.phases[0].flows.size() == 2);  // next == prev: no duplicate hop
  Schedule a = make_allpairs_schedule(8, Direction::Bi);
  EXPECT(a.phases.size() == 1);
  EXPECT(a.phases[0].flows.size() == 56);
  EXPECT(a.max_recv_slots() == 7);
  Schedule s1 = make_ring_schedule(1, Direction::Uni);
  EXPECT(all_flows(s1) == (std::multiset<std::pair<int, int>>{{0, 0}}));
  EXPECT(parse_mode("a2a") == Mode::AllPairs);
}

TEST(test_restrict_cells) {
  std::vector<std::pair<int, int>> cells{{0, 1}, {3, 2}};
  Schedule keep = make_pair_schedule(4, Direction::Uni);
  restrict_cells(&keep, cells, false);
  EXPECT(keep.phases.size() == 16);  // shape kept for the printed matrices
  EXPECT(validate(keep).empty());
  EXPECT(all_flows(keep) == (std::multiset<std::pair<int, int>>{{0, 1}, {3, 2}}));
  Schedule drop = make_pair_schedule(4, Direction::Uni);
  restrict_cells(&drop, cells, true);
  EXPECT(drop.phases.size() == 2);
  EXPECT(drop.phases[0].row == 0 && drop.phases[0].col == 1 && drop.phases[1].row == 3);
  Schedule ring = make_ring_schedule(4, Direction::Uni);
  restrict_cells(&ring, cells, true);
  EXPECT(ring.phases.size() == 1);  // other modes untouched
}

// ----------------------------------------------------------- placement ----

// ------------------------------------------------------------- routing ----

// Total bytes of a plan; checks that the stripes tile [0, total) without gaps
// or overlaps and that every stripe starts 4 KiB-aligned (direct stripe last
// in the message, first in the vector).
static size_t stripe_sum(const std::vector<Stripe>& v) {
  std::vector<std::pair<size_t, size_t>> spans;
  size_t s = 0;
  for (const auto& x : v) {
    spans.emplace_back(x.offset, x.bytes);
    s += x.bytes;
    EXPECT(x.offset % 4096 == 0);
  }
  EXPECT(!v.empty() && v[0].via == -1);
  std::sort(spans.begin(), spans.end());
  size_t off = 0;
  for (auto& sp : spans) {
    EXPECT(sp.first == off);
    off += sp.second;
  }
  EXPECT(v[0].offset + v[0].bytes == s);  // the direct stripe ends the message
  return s;
}

TEST(test_routes_single_pair_uses_every_relay) {
  const size_t bytes = 32u << 20;
  auto plan = plan_routes(8, {{0, 1}}, bytes);
  EXPECT(plan.size() == 1 && plan[0].size() == 7);
  EXPECT(plan[0][0].via == -1 && stripe_sum(plan[0]) == bytes);
  std::set<int> vias;
  for (size_t i = 1; i < plan[0].size(); ++i) {
    vias.insert(plan[0][i].via);
    EXPECT(plan[0][i].bytes % 4096 == 0);
    EXPECT(plan[0][i].bytes * 7 <= bytes && plan[0][i].bytes * 7 > bytes - 7 * 4096);  // equal shares
  }
  EXPECT((vias == std::set<int>{2, 3, 4, 5, 6, 7}));
  // Small messages, two ranks, weight 0 and max_relays 0 stay direct.
  EXPECT(plan_routes(8, {{0, 1}}, 64 << 10)[0].size() == 1);
  EXPECT(plan_routes(2, {{0, 1}}, bytes)[0].size() == 1);
  RouteOptions o;
  o.relay_weight = 0;
  EXPECT(plan_routes(8, {{0, 1}}, bytes, o)[0].size() == 1);
  o = RouteOptions();
  o.max_relays = 2;
  auto capped = plan_routes(8, {{0, 1}}, bytes, o);
  EXPECT(capped[0].size() == 3 && stripe_sum(capped[0]) == bytes);
}

TEST(test_routes_busy_links_and_duplicates) {
  const size_t bytes = 64u << 20;
  // All-pairs: every link carries a direct flow, nothing is relayed.
  std::vector<std::pair<int, int>> all;
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b)
      if (a != b) all.emplace_back(a, b);
  for (auto& p : plan_routes(4, all, bytes)) EXPECT(p.size() == 1 && p[0].bytes == bytes);
  // Bi-directional tournament round on 8 ranks: 6 relays per flow at half
  // the direct share (every relay link is shared by two segments).
  std::vector<std::pair<int, int>> round = {{0, 1}, {1, 0}, {2, 3}, {3, 2}, {4, 5}, {5, 4}, {6, 7}, {7, 6}};
  auto plan = plan_routes(8, round, bytes);
  std::map<std::pair<int, int>, int> seg;  // directed link -> segments
  for (size_t i = 0; i < round.size(); ++i) {
    EXPECT(plan[i].size() == 7 && stripe_sum(plan[i]) == bytes);
    EXPECT(plan[i][0].bytes > plan[i][1].bytes * 3 / 2);  // direct share 1 vs relay 1/2
    for (size_t j = 1; j < plan[i].size(); ++j) {
      const int k = plan[i][j].via;
      EXPECT(k != round[i].first && k != round[i].second);
      ++seg[{round[i].first, k}];
      ++seg[{k, round[i].second}];
    }
  }
  for (auto& kv : seg) EXPECT(kv.second <= 2);
  for (auto& f : round) EXPECT(seg.count(f) == 0);  // no relay over a direct flow's link
  // Duplicates plan identically; self flows stay whole.
  auto dup = plan_routes(8, {{0, 1}, {2, 2}, {0, 1}}, bytes);
  EXPECT(dup[0].size() == dup[2].size() && dup[0][1].bytes == dup[2][1].bytes);
  EXPECT(dup[1].size() == 1 && dup[1][0].bytes == bytes);
  // Unaligned sizes: every stripe still starts aligned; the tail is direct.
  for (size_t odd : {size_t{1822205}, (size_t{5} << 20) + 13}) {
    auto p = plan_routes(8, {{3, 1}}, odd);
    EXPECT(p[0].size() == 7 && stripe_sum(p[0]) == odd);
  }
}

TEST(test_host_hash_matches_reference) {
  // getHostHash (p2p_matrix.cc:44-51) computed by hand for "ab":
  // h0 = 5381; h1 = (5381*33) ^ 'a'; h2 = (h1*33) ^ 'b'
  uint64_t h = 5381;
  h = (h * 33) ^ 'a';
  h = (h * 33) ^ 'b';
  EXPECT(host_hash("ab") == h);
  EXPECT(host_hash("") == 5381);
  EXPECT(host_hash("node-1") != host_hash("node-2"));
}

TEST(test_placement) {
  std::vector<uint64_t> one(4, 7);
  Placement p = compute_placement(one, 3);
  EXPECT(p.ok && p.num_hosts == 1 && p.ranks_per_host == 4 && p.local_rank == 3);
  std::vector<uint64_t> blocks{1, 1, 2, 2};
  p = compute_placement(blocks, 3);
  EXPECT(p.ok && p.num_hosts == 2 && p.local_rank == 1 && p.host_index == 1);
  std::vector<uint64_t> rr{1, 2, 1, 2};  // round-robin placement is rejected
  p = compute_placement(rr, 0);
  EXPECT(!p.ok);
  EXPECT(p.error.find("block") != std::string::npos);
  std::vector<uint64_t> uneven{1, 1, 2};
  EXPECT(!compute_placement(uneven, 0).ok);
}

// ----------------------------------------------------------------- prng ----

TEST(test_prng_fill_verify) {
  for (size_t bytes : {size_t(1), size_t(3), size_t(4), size_t(15), size_t(16), size_t(17), size_t(4096), size_t(4099), size_t(1 << 20)}) {
    std::vector<uint8_t> buf(bytes + 8, 0xEE);
    host_fill(buf.data(), bytes, 42);
    EXPECT(buf[bytes] == 0xEE);  // no overrun
    VerifyResult r = host_verify(buf.data(), bytes, 42);
    EXPECT(r.mismatches == 0);
    EXPECT(r.first_bad == ~0ull);
    VerifyResult w = host_verify(buf.data(), bytes, 43);
    EXPECT(bytes < 4 ? w.mismatches <= 1 : w.mismatches > 0);
    if (bytes >= 16) {
      buf[bytes / 2] ^= 0x10;
      VerifyResult c = host_verify(buf.data(), bytes, 42);
      EXPECT(c.mismatches == 1);
      EXPECT(c.first_bad == (bytes / 2) / 4 * 4);
    }
  }
  // Words are a function of (seed, index) only.
  EXPECT(prng_word(1, 0) != prng_word(2, 0));
  EXPECT(prng_word(1, 5) == prng_word(1, 5));
  EXPECT(prng_word(1, 1ull << 32) != prng_word(1, 0));
  EXPECT(payload_seed(0, 4096, 0) != payload_seed(1, 4096, 0));
  EXPECT(payload_seed(0, 4096, 0) != payload_seed(0, 8192, 0));
  // Known-answer vector pinned for cross-language checks (tests/test_prng.py).
  std::printf("    prng_word(0x1234, 0..3) = %08x %08x %08x %08x\n", prng_word(0x1234, 0), prng_word(0x1234, 1),
              prng_word(0x1234, 2), prng_word(0x1234, 3));
}

TEST(test_checksum_convention) {
  uint8_t b[6] = {1, 0, 0, 0, 2, 3};
  VerifyResult r = host_verify(b, 6, 0);
  EXPECT(r.checksum == 1u + (2u | (3u << 8)));
}

// --------------------------------------------------------------- report ----

static std::string capture(const std::function<void(FILE*)>& fn) {
  char* buf = nullptr;
  size_t len = 0;
  FILE* f = open_memstream(&buf, &len);
  fn(f);
  std::fclose(f);
  std::string s(buf, len);
  std::free(buf);
  return s;
}

static PhaseResult fake_cell(int row, int col, double gbps_value) {
  PhaseResult r;
  r.row = row;
  r.col = col;
  r.idle = row == col;
  r.seconds_per_iter = 1.0;
  r.bytes_per_iter = gbps_value * 1e9 / 8.0;
  return r;
}

TEST(test_compat_golden) {
  // SURVEY.md Appendix B, generated from the reference's printf sequence.
  const std::string golden =
      "Evaluating the Uni-Directional NCCL P2P Bandwidth (Gbps)\n"
      "   D\\D     0      1 \n"
      "     0   0.00 391.53 \n"
      "     1 1234.50   0.00 \n"
      "\n"
      "Evaluating the Bi-Directional NCCL P2P Bandwidth (Gbps)\n"
      "   D\\D     0      1 \n"
      "     0   0.00 391.53 \n"
      "     1 1234.50   0.00 \n";
  std::string got = capture([](FILE* f) {
    CompatPrinter cp(f, 2);
    for (Direction d : {Direction::Uni, Direction::Bi}) {
      cp.begin(d, false);
      cp.on_phase(fake_cell(0, 0, 0));
      cp.on_phase(fake_cell(0, 1, 391.53));
      cp.on_phase(fake_cell(1, 0, 1234.5));
      cp.on_phase(fake_cell(1, 1, 0));
    }
  });
  EXPECT(got == golden);
  if (got != golden) std::fprintf(stderr, "got:\n%s\n", got.c_str());
}

TEST(test_json_escape) {
  EXPECT(json_escape("a\"b\\c\n") == "a\\\"b\\\\c\\n");
}

TEST(test_repeat_summaries) {
  // --repeat: per (mode, dir, size) every run's mean cell (pair: the compat
  // cell / 8, bi both directions summed) and their median / min / max.
  auto pair_run = [](Direction d, double gbps01, double gbps10, int rep) {
    RunRecord r;
    r.mode = Mode::Pair;
    r.dir = d;
    r.bytes = 1 << 20;
    r.repeat = rep;
    for (int i = 0; i < 2; ++i) {
      PhaseResult ph;
      ph.row = i;
      ph.col = 1 - i;
      ph.seconds_per_iter = 1.0;
      ph.bytes_per_iter = (i == 0 ? gbps01 : gbps10) * 1e9 / 8.0;
      r.phases.push_back(ph);
    }
    return r;
  };
  std::vector<RunRecord> runs = {pair_run(Direction::Uni, 80, 160, 0), pair_run(Direction::Uni, 40, 40, 1),
                                 pair_run(Direction::Bi, 200, 200, 0), pair_run(Direction::Uni, 800, 800, 2)};
  auto s = repeat_summaries(runs, 2);
  EXPECT(s.size() == 2 && s[0].dir == Direction::Uni && s[1].dir == Direction::Bi);
  EXPECT(s[0].runs.size() == 3 && std::fabs(s[0].runs[0] - 15.0) < 1e-9 && std::fabs(s[0].runs[1] - 5.0) < 1e-9);
  EXPECT(std::fabs(s[0].median - 15.0) < 1e-9 && std::fabs(s[0].min - 5.0) < 1e-9 && std::fabs(s[0].max - 100.0) < 1e-9);
  EXPECT(s[1].runs.size() == 1 && std::fabs(s[1].median - 25.0) < 1e-9);
  const std::string js = repeat_summary_json(s[0]);
  EXPECT(js.find("\"type\":\"repeats\"") != std::string::npos && js.find("\"median\":15") != std::string::npos);
}

TEST(test_cli_defaults_match_reference) {
  AppConfig cfg;
  int code = -1;
  char prog_args[1][1] = {{0}};
  (void)prog_args;
  EXPECT(parse_cli(0, nullptr, &cfg, &code));
  EXPECT(cfg.modes.size() == 1 && cfg.modes[0] == Mode::Pair);
  EXPECT(cfg.dirs.size() == 2 && cfg.dirs[0] == Direction::Uni && cfg.dirs[1] == Direction::Bi);
  EXPECT(cfg.sizes.size() == 1 && cfg.sizes[0] == (32u << 20));
  EXPECT(cfg.run.iters == 128);
  std::vector<std::string> args{"--mode", "ring,allpairs", "--sizes", "4K:16K", "-n", "auto", "--reference", "--dir=bi"};
  std::vector<char*> argv;
  for (auto& a : args) argv.push_back(&a[0]);
  AppConfig c2;
  EXPECT(parse_cli(static_cast<int>(argv.size()), argv.data(), &c2, &code));
  EXPECT(c2.modes.size() == 2 && c2.modes[1] == Mode::AllPairs);
  EXPECT(c2.sizes.size() == 3);
  EXPECT(c2.iters_auto);
  EXPECT(c2.run.timing == Timing::Wallclock && c2.run.warmup == 0 && !c2.warm_connections);
  EXPECT(c2.reference_buffers && !cfg.reference_buffers);  // one send / receive region, like p2p_matrix.cc:124-130
  EXPECT(c2.dirs.size() == 1 && c2.dirs[0] == Direction::Bi);
  EXPECT(auto_iters(32u << 20, 4ull << 30) == 128);  // the reference's 128 x 32 MiB
  EXPECT(auto_iters(4096, 4ull << 30) == 1000);
  EXPECT(auto_iters(4ull << 30, 4ull << 30) == 8);
}

TEST(test_cli_verify_impl_names) {
  // Round 5 kept the LDS-DMA (lds8) and the register (stride) verify: the
  // older names of each staging are aliases.
  const std::pair<const char*, int> known[] = {{"auto", 0}, {"lds8", 1},   {"lds", 1},     {"stride", 2},
                                               {"reg", 2},  {"register", 2}};
  for (const auto& [name, impl] : known) {
    std::vector<std::string> args{"--verify-impl", name};
    std::vector<char*> argv;
    for (auto& a : args) argv.push_back(&a[0]);
    AppConfig cfg;
    int code = -1;
    EXPECT(parse_cli(static_cast<int>(argv.size()), argv.data(), &cfg, &code) && cfg.verify_impl == impl);
  }
  // A misspelt name is an error, not a silent fall-back to the default.
  std::vector<std::string> args{"--verify-impl", "lds8span"};
  std::vector<char*> argv;
  for (auto& a : args) argv.push_back(&a[0]);
  AppConfig cfg;
  int code = -1;
  EXPECT(!parse_cli(static_cast<int>(argv.size()), argv.data(), &cfg, &code) && code == 1);
  // A removed variant says so (and which profile holds its numbers).
  for (const char* gone : {"lds-cached", "lds-pipe", "lds8-span", "grid"}) {
    std::string note;
    EXPECT(parse_verify_impl(gone, &note) == -2 && note.find("removed in round 5") != std::string::npos &&
           note.find("profiles/") != std::string::npos);
    std::vector<std::string> a2{"--verify-impl", gone};
    std::vector<char*> v2;
    for (auto& x : a2) v2.push_back(&x[0]);
    AppConfig c2;
    int code2 = -1;
    EXPECT(!parse_cli(static_cast<int>(v2.size()), v2.data(), &c2, &code2) && code2 == 1);
  }
  std::string note;
  EXPECT(parse_verify_impl("lds8span", &note) == -1 && note.find("unknown") != std::string::npos);
}

// ------------------------------------------- multi-rank engine (threads) ----

static void run_ranks(int n, const std::function<void(Bootstrap&, Transport&)>& body, bool shm = false) {
  TcpListener listener(0, "127.0.0.1");
  int port = listener.port();
  std::vector<std::thread> th;
  for (int r = 0; r < n; ++r) {
    th.emplace_back([&, r]() {
      auto boot = make_tcp_bootstrap(r, n, "127.0.0.1", port, 60.0, r == 0 ? &listener : nullptr);
      TransportOptions opt;
      opt.timeout_s = 60;
      auto t = shm ? make_shm_transport(*boot, opt) : make_host_transport(*boot, opt);
      body(*boot, *t);
    });
  }
  for (auto& t : th) t.join();
}

TEST(test_bootstrap_collectives) {
  run_ranks(4, [](Bootstrap& b, Transport&) {
    auto v = b.allgather_value(b.rank() * 10);
    EXPECT(v.size() == 4 && v[3] == 30);
    int x = b.rank() == 2 ? 77 : 0;
    b.bcast(&x, sizeof(x), 2);
    EXPECT(x == 77);
    EXPECT(b.allreduce_max(static_cast<double>(b.rank())) == 3.0);
    EXPECT(b.allreduce_sum_u64(1) == 4);
    b.barrier();
  });
}

TEST(test_engine_all_modes_host_transport) {
  const int n = 4;
  std::vector<uint64_t> mism(n, 1);
  run_ranks(n, [&](Bootstrap& b, Transport& t) {
    uint64_t bad = 0;
    for (Mode m : {Mode::Pair, Mode::Ring, Mode::AllPairs, Mode::Tournament, Mode::Self}) {
      for (Direction d : {Direction::Uni, Direction::Bi}) {
        Schedule s = make_schedule(m, d, n);
        RunConfig cfg;
        cfg.bytes = 4099;  // odd size exercises the tail path
        cfg.iters = 3;
        cfg.warmup = 1;
        cfg.verify = true;
        Buffers bufs(t, cfg.bytes, std::max(1, s.max_recv_slots()));
        auto res = run_schedule(t, b, s, cfg, bufs);
        EXPECT(res.size() == s.phases.size());
        for (auto& ph : res) {
          bad += ph.total_mismatches;
          if (!ph.idle) {
            EXPECT(ph.seconds_per_iter > 0);
            for (auto& f : ph.flows) EXPECT(f.verified && f.gbs > 0);
          }
        }
      }
    }
    mism[b.rank()] = bad;
  });
  for (auto v : mism) EXPECT(v == 0);
}

TEST(test_engine_receive_generations) {
  // Every timed iteration in a generation of its own (RunConfig::gens): the
  // engine checks iters x receivers deliveries, each generation against its
  // own PRNG stream; the budget caps the generations (256 MiB where the
  // transport cannot tell free memory: 64 KiB slots -> 2048 generations).
  const int n = 3;
  std::vector<int> ok(n, 0);
  run_ranks(n, [&](Bootstrap& b, Transport& t) {
    Schedule s = make_schedule(Mode::Tournament, Direction::Bi, n);
    RunConfig cfg;
    cfg.bytes = 65536;
    cfg.iters = 5;
    cfg.warmup = 2;
    cfg.verify = true;
    cfg.gens = verify_generations(t, b, cfg.bytes, s.max_recv_slots(), cfg.iters);
    EXPECT(cfg.gens == 5);  // min(iters, budget / (64 KiB x (slots + 1)))
    Buffers bufs(t, cfg.bytes, s.max_recv_slots() * cfg.gens, slot_stride_bytes(cfg.bytes) * static_cast<size_t>(cfg.gens));
    auto res = run_schedule(t, b, s, cfg, bufs);
    bool good = true;
    for (auto& ph : res) {
      if (ph.idle) continue;
      good = good && ph.generations == 5 && ph.total_mismatches == 0 && ph.timed_msgs == ph.verified_msgs &&
             ph.timed_msgs == 5 * ph.flows.size() && ph.op_bytes == 0 && ph.rechunked_to.empty();
    }
    // Generations draw from distinct PRNG streams.
    good = good && generation_seed(1, 4096, 7, 0) != generation_seed(1, 4096, 7, 1) &&
           generation_seed(1, 4096, 7, 0) == payload_seed(1, 4096, 7);
    ok[b.rank()] = good ? 1 : 0;
  });
  for (int v : ok) EXPECT(v == 1);
}

TEST(test_engine_all_modes_shm_transport) {
  // Same engine over the shared-memory rings: every mode, odd sizes, and a
  // message larger than the ring (wraps and back-pressure).
  const int n = 4;
  std::vector<uint64_t> mism(n, 1);
  run_ranks(n, [&](Bootstrap& b, Transport& t) {
    EXPECT(t.name() == "shm");
    uint64_t bad = 0;
    for (size_t bytes : {size_t{4099}, size_t{3} << 20}) {
      for (Mode m : {Mode::Pair, Mode::Ring, Mode::AllPairs, Mode::Tournament, Mode::Self}) {
        for (Direction d : {Direction::Uni, Direction::Bi}) {
          Schedule s = make_schedule(m, d, n);
          RunConfig cfg;
          cfg.bytes = bytes;
          cfg.iters = 2;
          cfg.warmup = 1;
          cfg.verify = true;
          Buffers bufs(t, cfg.bytes, std::max(1, s.max_recv_slots()));
          auto res = run_schedule(t, b, s, cfg, bufs);
          for (auto& ph : res) {
            bad += ph.total_mismatches;
            if (!ph.idle)
              for (auto& f : ph.flows) EXPECT(f.verified && f.gbs > 0);
          }
        }
      }
    }
    auto lat = run_latency(t, b, 4096, 50, 5, *std::make_unique<Buffers>(t, 4096, 1));
    EXPECT(lat.size() == 6);
    for (auto& l : lat) EXPECT(l.one_way_us.p50 > 0);
    mism[b.rank()] = bad;
  }, true);
  for (auto v : mism) EXPECT(v == 0);
}

// A transport that asks for the group's global flows (like the IPC relay
// engine) on top of the host transport: every rank must then post every
// group, and every rank must see the same flow list in the same order.
class FlowRecorder final : public Transport {
 public:
  explicit FlowRecorder(Transport& t) : t_(&t) {}
  std::string name() const override { return "flow-recorder"; }
  int rank() const override { return t_->rank(); }
  int nranks() const override { return t_->nranks(); }
  void* alloc(size_t b) override { return t_->alloc(b); }
  void release(void* p) override { t_->release(p); }
  void fill(void* p, size_t b, uint64_t s) override { t_->fill(p, b, s); }
  void zero(void* p, size_t b) override { t_->zero(p, b); }
  VerifyResult verify(const void* p, size_t b, uint64_t s) override { return t_->verify(p, b, s); }
  void group_begin() override {
    ++groups;
    t_->group_begin();
  }
  void send(const void* p, size_t b, int peer) override { t_->send(p, b, peer); }
  void recv(void* p, size_t b, int peer) override { t_->recv(p, b, peer); }
  void group_end() override { t_->group_end(); }
  int mark() override { return t_->mark(); }
  double elapsed_ms(int a, int b) override { return t_->elapsed_ms(a, b); }
  void clear_marks() override { t_->clear_marks(); }
  void sync() override { t_->sync(); }
  bool wants_group_flows() const override { return true; }
  void group_flows(const void*, const std::vector<GroupFlow>& flows, size_t bytes) override {
    for (const auto& f : flows) log.push_back({f.src, f.dst, f.slot, static_cast<int>(bytes & 0x7fffffff)});
  }
  std::vector<std::array<int, 4>> log;
  long groups = 0;

 private:
  Transport* t_;
};

TEST(test_group_flows_posted_on_every_rank) {
  const int n = 4;
  std::vector<std::vector<std::array<int, 4>>> logs(n);
  std::vector<long> groups(n, 0);
  run_ranks(n, [&](Bootstrap& b, Transport& host) {
    FlowRecorder t(host);
    uint64_t bad = 0;
    for (Mode m : {Mode::Pair, Mode::Tournament, Mode::Ring}) {
      Schedule s = make_schedule(m, Direction::Uni, n);
      RunConfig cfg;
      cfg.bytes = 8192;
      cfg.iters = 2;
      cfg.warmup = 1;
      cfg.verify = true;
      Buffers bufs(t, cfg.bytes, std::max(1, s.max_recv_slots()));
      for (auto& ph : run_schedule(t, b, s, cfg, bufs)) bad += ph.total_mismatches;
    }
    StepDriver d(t, b, make_tournament_schedule(n, Direction::Bi), 4096, 2, true);
    d.connect();
    for (long k = 0; k < 3; ++k) d.step(k);
    d.sync();
    EXPECT(d.verify_last() == 0 && bad == 0);
    logs[b.rank()] = t.log;
    groups[b.rank()] = t.groups;
    b.barrier();
  });
  for (int r = 1; r < n; ++r) {
    EXPECT(logs[r] == logs[0]);      // same flows, same order, on every rank
    EXPECT(groups[r] == groups[0]);  // pair cells: idle ranks post too
  }
  EXPECT(!logs[0].empty());
  // Every logged flow names a real receive slot on its receiver.
  for (const auto& e : logs[0]) EXPECT(e[0] != e[1] && e[2] >= 0);
}

// Transport-level fuzz (runner.cpp fuzz_transport): random groups of
// messages, self and repeated pairs included, sizes up to twice the shm ring.
static void fuzz_transport_test(bool shm) {
  const int n = 4;
  std::vector<uint64_t> bad(n, 1);
  run_ranks(n, [&](Bootstrap& b, Transport& t) { bad[b.rank()] = fuzz_transport(t, b, 40, 0x5EED, size_t{2} << 20); }, shm);
  for (auto v : bad) EXPECT(v == 0);
}

TEST(test_fuzz_host_transport) { fuzz_transport_test(false); }
TEST(test_fuzz_shm_transport) { fuzz_transport_test(true); }

TEST(test_wallclock_and_latency_host) {
  run_ranks(3, [&](Bootstrap& b, Transport& t) {
    Schedule s = make_pair_schedule(3, Direction::Bi);
    RunConfig cfg;
    cfg.bytes = 4096;
    cfg.iters = 4;
    cfg.warmup = 0;
    cfg.timing = Timing::Wallclock;
    Buffers bufs(t, 4096, 1);
    auto res = run_schedule(t, b, s, cfg, bufs);
    for (auto& ph : res)
      if (!ph.idle) EXPECT(ph.seconds_per_iter > 0 && ph.flows.size() == 2);
    auto lat = run_latency(t, b, 8, 20, 2, bufs);
    EXPECT(lat.size() == 3);
    for (auto& l : lat) EXPECT(l.one_way_us.n == 20 && l.one_way_us.p50 > 0);
  });
}

TEST(test_preposted_latency_batches) {
  // Without a gate the pre-posted ping-pong falls back to host-posted samples;
  // with one (faked on the CPU) it runs in batches whose first exchange is not
  // sampled, and still yields exactly `iters` samples per pair.
  for (int fake : {0, 1}) {
    setenv("P2P_TEST_FAKE_GATE", fake ? "1" : "0", 1);
    run_ranks(4, [&](Bootstrap& b, Transport& t) {
      Buffers bufs(t, 64, 1);
      auto lat = run_latency(t, b, 8, 37, 2, bufs, 8);
      EXPECT(lat.size() == 6);
      for (auto& l : lat) {
        EXPECT(l.method == (fake ? "preposted" : "host"));
        EXPECT(l.one_way_us.n == 37 && l.one_way_us.p50 > 0);
      }
    });
  }
  unsetenv("P2P_TEST_FAKE_GATE");
}

TEST(test_step_driver_host) {
  run_ranks(4, [&](Bootstrap& b, Transport& t) {
    StepDriver d(t, b, make_tournament_schedule(4, Direction::Bi), 8192, 2, true);
    d.connect();
    for (long k = 0; k < 6; ++k) d.step(k);
    d.sync();
    auto ms = d.step_ms();
    EXPECT(ms.size() == 6);
    EXPECT(d.verify_last() == 0);
    EXPECT(d.job_bytes_per_step(0) == 4.0 * 8192 * 2);
    EXPECT(d.bytes_sent_per_step(0) == 8192.0 * 2);
    b.barrier();
    // Batched posting (one group per step) and a graph request on a
    // transport without graphs (ignored) must move the same data.
    StepOptions so;
    so.batch = true;
    so.graph = true;
    StepDriver bd(t, b, make_ring_schedule(4, Direction::Bi), 4099, 3, true, 7, so);
    bd.connect();
    for (long k = 0; k < 3; ++k) bd.step(k);
    bd.sync();
    EXPECT(bd.verify_last() == 0);
    b.barrier();
  });
}

// Verification covers the timed steps: every message of every step has its
// own slot (and payload region), poison() clears them, and verify_steps()
// accepts only slots the steps after poison() wrote.
TEST(test_step_driver_verifies_timed_steps) {
  for (bool shm : {false, true})
    run_ranks(4, [&](Bootstrap& b, Transport& t) {
      const int steps = 7;  // 2 laps + 1 step of the 3 tournament rounds
      StepOptions so;
      so.batch = true;
      so.depth = 3;
      StepDriver d(t, b, make_tournament_schedule(4, Direction::Bi), 4100, 3, true, 11, so);
      EXPECT(d.depth() == 3);
      // Slots are distinct across (generation, phase, message, sender).
      std::vector<int> seen;
      for (int g = 0; g < 3; ++g)
        for (int p = 0; p < 3; ++p)
          for (int m = 0; m < 3; ++m) seen.push_back(d.slot_index(b.rank(), g, p, m, 0));
      std::sort(seen.begin(), seen.end());
      EXPECT(std::unique(seen.begin(), seen.end()) == seen.end());
      EXPECT(d.msg_seed(0, 0) != d.msg_seed(0, 1) && d.msg_seed(0, 0) != d.msg_seed(1, 0));
      d.connect();
      for (long k = 0; k < 2; ++k) d.step(k);  // warmup
      d.sync();
      d.poison();
      d.run_steps(2, steps);  // chained marks: one per step boundary
      d.sync();
      {
        auto ms = d.step_ms();
        EXPECT(ms.size() == static_cast<size_t>(2 + steps));
        for (double v : ms) EXPECT(v >= 0);
      }
      StepVerifyReport r = d.verify_steps(2, steps);
      EXPECT(r.mismatches == 0);
      // 4 ranks x 1 sender x 3 messages per step.
      EXPECT(r.timed_msgs == static_cast<uint64_t>(steps) * 4 * 3);
      EXPECT(r.verified_msgs == r.timed_msgs);  // depth 3 >= 3 laps: nothing overwritten
      // Poisoned and never written again: every slot fails.
      d.poison();
      StepVerifyReport z = d.verify_steps(2, steps);
      EXPECT(z.mismatches == static_cast<uint64_t>(z.slots) * ((4100 + 3) / 4));
      // Depth 1: later laps overwrite earlier ones; coverage says so.
      StepOptions s1;
      s1.depth = 1;
      StepDriver d1(t, b, make_tournament_schedule(4, Direction::Bi), 4096, 2, true, 12, s1);
      d1.connect();
      d1.poison();
      for (long k = 0; k < 6; ++k) d1.step(k);
      d1.sync();
      StepVerifyReport r1 = d1.verify_steps(0, 6);
      EXPECT(r1.mismatches == 0 && r1.timed_msgs == 6u * 4 * 2 && r1.verified_msgs == 3u * 4 * 2);
      b.barrier();
    }, shm);
}

// A step posted in groups of whole messages (the first step of a run, or
// every step) moves and verifies exactly what one group per step does.
TEST(test_step_driver_split_groups) {
  for (int mode = 0; mode < 2; ++mode)
    run_ranks(4, [&](Bootstrap& b, Transport& t) {
      StepOptions so;
      so.batch = true;
      so.depth = 3;
      (mode == 0 ? so.first_group_msgs : so.group_msgs) = 2;
      StepDriver d(t, b, make_tournament_schedule(4, Direction::Bi), 4100, 5, true, 13, so);
      d.connect();
      d.poison();
      d.run_steps(0, 9);
      d.sync();
      StepVerifyReport r = d.verify_steps(0, 9);
      EXPECT(r.mismatches == 0);
      EXPECT(r.timed_msgs == 9u * 4 * 5 && r.verified_msgs == r.timed_msgs);
      EXPECT(d.post_ms().size() == 9u);
      b.barrier();
    }, mode == 1);
}

// ------------------------------------ reported times on a scripted clock ----
//
// The engine's arithmetic on marks (run_phase, run_latency, StepDriver) with
// a transport that moves the data through the host transport but owns time:
// mark() returns the ordinal j of the mark since the last clear_marks(), and
// rank r's mark j lies at T_r(j) = sum_{i<j} d_r(i) milliseconds with
// d_r(i) = (r + 1) * (1 + (5 i mod 7)) / 64.  Every value and partial sum is
// exact in a double; the steps are irregular, so a mark paired with the wrong
// neighbour shows; ranks differ, so the slower endpoint is decidable.  The
// expected values below come from T_r by plain loops (summarize, which has
// its own test, is applied to the expected sample list).

static double script_step_ms(int r, long i) { return (r + 1) * static_cast<double>(1 + (5 * i) % 7) / 64.0; }
static double script_T(int r, long j) {
  double t = 0;
  for (long i = 0; i < j; ++i) t += script_step_ms(r, i);
  return t;
}

class ScriptedClock final : public Transport {
 public:
  explicit ScriptedClock(Transport& t, int concurrency = 1, bool relay = false) : t_(&t), k_(concurrency), relay_(relay) {}
  std::string name() const override { return "scripted-clock"; }
  int rank() const override { return t_->rank(); }
  int nranks() const override { return t_->nranks(); }
  void* alloc(size_t b) override { return t_->alloc(b); }
  void release(void* p) override { t_->release(p); }
  void fill(void* p, size_t b, uint64_t s) override { t_->fill(p, b, s); }
  void zero(void* p, size_t b) override { t_->zero(p, b); }
  VerifyResult verify(const void* p, size_t b, uint64_t s) override { return t_->verify(p, b, s); }
  void group_begin() override { t_->group_begin(); }
  void send(const void* p, size_t b, int peer) override { t_->send(p, b, peer); }
  void recv(void* p, size_t b, int peer) override { t_->recv(p, b, peer); }
  void group_end() override {
    t_->group_end();
    log += 'g';
  }
  bool gate_arm(double s) override { return t_->gate_arm(s); }
  void gate_release() override { t_->gate_release(); }
  bool gate_timed_out() override { return t_->gate_timed_out(); }
  bool wants_group_flows() const override { return relay_; }
  int mark() override {
    log += 'm';
    return next_++;
  }
  double elapsed_ms(int a, int b) override {
    asked.emplace_back(a, b);
    return script_T(rank(), b) - script_T(rank(), a);
  }
  void clear_marks() override {
    log += 'c';
    next_ = 0;
  }
  int concurrency() const override { return k_; }
  void sync() override {
    t_->sync();
    log += 's';
  }
  long count(char what) const { return std::count(log.begin(), log.end(), what); }

  std::string log;                         // c(lear) m(ark) g(roup_end) s(ync), in order
  std::vector<std::pair<int, int>> asked;  // every elapsed_ms(a, b), in order

 private:
  Transport* t_;
  int k_;
  bool relay_;  // asks for every group's flows: ranks outside a phase post and time it too
  int next_ = 0;
};

static bool rel_eq(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::max(std::fabs(a), std::fabs(b)); }
#define EXPECT_REL(a, b) EXPECT(rel_eq((a), (b)))

static void expect_summary(const Summary& got, const std::vector<double>& want_samples) {
  const Summary w = summarize(want_samples);
  EXPECT(got.n == w.n);
  EXPECT_REL(got.min, w.min);
  EXPECT_REL(got.max, w.max);
  EXPECT_REL(got.mean, w.mean);
  EXPECT_REL(got.stdev, w.stdev);
  EXPECT_REL(got.p50, w.p50);
  EXPECT_REL(got.p90, w.p90);
  EXPECT_REL(got.p99, w.p99);
}

static std::string repeat(const std::string& s, int n) {
  std::string o;
  for (int i = 0; i < n; ++i) o += s;
  return o;
}

struct ScriptedRun {
  PhaseResult res;
  std::string log;
  std::vector<std::pair<int, int>> asked;
};

// One phase on n ranks over the scripted clock; what every rank got.
static std::vector<ScriptedRun> scripted_phase(int n, const Phase& phase, const RunConfig& cfg, int concurrency = 1,
                                               bool relay = false) {
  std::vector<ScriptedRun> out(static_cast<size_t>(n));
  run_ranks(n, [&](Bootstrap& b, Transport& host) {
    ScriptedClock t(host, concurrency, relay);
    Buffers bufs(t, cfg.bytes, std::max(1, phase.max_recv_slots()));
    ScriptedRun& r = out[static_cast<size_t>(b.rank())];
    r.res = run_phase(t, b, phase, 0, cfg, bufs);
    r.log = t.log;
    r.asked = t.asked;
    b.barrier();
  });
  return out;
}

static RunConfig scripted_config(int iters, int warmup) {
  RunConfig cfg;
  cfg.bytes = 4100;
  cfg.iters = iters;
  cfg.warmup = warmup;
  cfg.verify = true;
  return cfg;
}

// The numbers of an events-timed phase that follow from each rank's scripted
// time `T_r(last)` over its timed window: rank_seconds, the flows' seconds and
// rates, the phase's seconds and rates.
static void expect_phase_numbers(const PhaseResult& res, const Phase& phase, const RunConfig& cfg, long last) {
  const int n = static_cast<int>(phase.ranks.size());
  const double iters = cfg.iters;
  EXPECT(res.rank_seconds.size() == static_cast<size_t>(n));
  double slowest = 0;
  for (int r = 0; r < n; ++r) {
    const double want = phase.participates(r) ? script_T(r, last) / 1e3 : 0.0;
    EXPECT_REL(res.rank_seconds[static_cast<size_t>(r)], want);
    slowest = std::max(slowest, want);
  }
  EXPECT(slowest > 0);
  EXPECT_REL(res.seconds_per_iter, slowest / iters);
  const double bytes = static_cast<double>(cfg.bytes);
  EXPECT(res.bytes_per_iter == bytes * static_cast<double>(phase.flows.size()));
  EXPECT_REL(res.agg_gbs, bytes * static_cast<double>(phase.flows.size()) / (slowest / iters) / 1e9);
  EXPECT(res.flows.size() == phase.flows.size());
  for (size_t i = 0; i < res.flows.size() && i < phase.flows.size(); ++i) {
    const FlowResult& f = res.flows[i];
    EXPECT(f.flow == phase.flows[i]);
    const double s = std::max(script_T(f.flow.src, last), script_T(f.flow.dst, last)) / 1e3 / iters;
    EXPECT_REL(f.seconds, s);
    EXPECT_REL(f.gbs, bytes / s / 1e9);
    EXPECT_REL(f.gbps, 8.0 * bytes / s / 1e9);
    EXPECT(f.verified && f.mismatches == 0);
  }
}

TEST(test_scripted_run_phase_events) {
  const int n = 4, iters = 10, warmup = 3;
  const Phase phase = make_tournament_schedule(n, Direction::Bi).phases[0];
  EXPECT(phase.flows.size() == 4);
  const RunConfig cfg = scripted_config(iters, warmup);
  const auto runs = scripted_phase(n, phase, cfg);
  for (int me = 0; me < n; ++me) {
    const ScriptedRun& run = runs[static_cast<size_t>(me)];
    // One mark before the first timed group and one after each; the warmup's
    // groups lie before the clear and carry no mark.
    const size_t clear = run.log.rfind('c');
    EXPECT(clear != std::string::npos);
    if (clear == std::string::npos) continue;
    EXPECT(run.log.substr(clear + 1) == "m" + repeat("gm", iters) + "s");
    const std::string before = run.log.substr(0, clear);
    EXPECT(std::count(before.begin(), before.end(), 'g') == warmup);
    EXPECT(before.find('m') == std::string::npos && before.find('c') == std::string::npos);
    EXPECT(!before.empty() && before.back() == 's');  // the warmup was waited for before the window opened

    expect_phase_numbers(run.res, phase, cfg, iters);
    // The pair without rank 3 is not charged rank 3's time.
    int without3 = 0;
    for (const FlowResult& f : run.res.flows) {
      if (f.flow.src == 3 || f.flow.dst == 3) continue;
      ++without3;
      EXPECT(f.seconds < script_T(3, iters) / 1e3 / iters);
      EXPECT_REL(f.seconds, script_T(std::max(f.flow.src, f.flow.dst), iters) / 1e3 / iters);
    }
    EXPECT(without3 == 2);
    EXPECT_REL(run.res.seconds_per_iter, script_T(3, iters) / 1e3 / iters);
    // iter_us of a -> b: the receiver's mark-to-mark intervals.
    for (const FlowResult& f : run.res.flows) {
      std::vector<double> want;
      for (long i = 0; i < iters; ++i) want.push_back((script_T(f.flow.dst, i + 1) - script_T(f.flow.dst, i)) * 1e3);
      expect_summary(f.iter_us, want);
    }
  }
}

TEST(test_scripted_run_phase_concurrency_and_no_samples) {
  const int n = 4, k = 4;
  const Phase phase = make_tournament_schedule(n, Direction::Bi).phases[0];
  // K messages in flight: a sample spans K marks and is divided by K; the
  // marks left over after the last full round go into none; fewer than K
  // marks give one averaged sample.
  for (int iters : {10, 3, 8}) {
    const RunConfig cfg = scripted_config(iters, 1);
    const auto runs = scripted_phase(n, phase, cfg, k);
    for (int me = 0; me < n; ++me) {
      const ScriptedRun& run = runs[static_cast<size_t>(me)];
      expect_phase_numbers(run.res, phase, cfg, iters);  // the window does not depend on the grouping
      for (const FlowResult& f : run.res.flows) {
        const int d = f.flow.dst;
        std::vector<double> want;
        if (iters == 10)
          want = {(script_T(d, 4) - script_T(d, 0)) * 1e3 / 4, (script_T(d, 8) - script_T(d, 4)) * 1e3 / 4};
        else if (iters == 3)
          want = {script_T(d, 3) * 1e3 / 3};
        else
          want = {(script_T(d, 4) - script_T(d, 0)) * 1e3 / 4, (script_T(d, 8) - script_T(d, 4)) * 1e3 / 4};
        expect_summary(f.iter_us, want);
        if (iters == 8)  // two samples that tile the window
          EXPECT_REL(f.iter_us.mean * 2 * 4, script_T(d, 8) * 1e3);
      }
    }
  }
  // samples off: a mark before the first group and one after the last.
  RunConfig cfg = scripted_config(10, 3);
  cfg.samples = false;
  const auto runs = scripted_phase(n, phase, cfg);
  for (int me = 0; me < n; ++me) {
    const ScriptedRun& run = runs[static_cast<size_t>(me)];
    const size_t clear = run.log.rfind('c');
    EXPECT(clear != std::string::npos);
    if (clear == std::string::npos) continue;
    EXPECT(run.log.substr(clear + 1) == "m" + repeat("g", 10) + "m" + "s");
    expect_phase_numbers(run.res, phase, cfg, 1);  // the two marks are ordinals 0 and 1
    for (const FlowResult& f : run.res.flows) EXPECT(f.iter_us.n == 0);
  }
}

TEST(test_scripted_run_phase_non_participant) {
  const int n = 3, iters = 10;
  const Schedule s = make_pair_schedule(n, Direction::Uni);
  const RunConfig cfg = scripted_config(iters, 2);
  int cells = 0, idle = 0;
  for (const Phase& phase : s.phases) {
    if (phase.idle) {
      // The diagonal reports 0 and posts nothing.
      if (idle++ > 0) continue;
      for (const ScriptedRun& run : scripted_phase(n, phase, cfg)) {
        EXPECT(run.res.idle && run.res.seconds_per_iter == 0 && run.res.agg_gbs == 0 && run.res.flows.empty());
        for (double v : run.res.rank_seconds) EXPECT(v == 0);
        EXPECT(run.log.empty() && run.asked.empty());
      }
      continue;
    }
    if (!(phase.row == 0 && phase.col == 1) && !(phase.row == 2 && phase.col == 0)) continue;
    ++cells;
    const int out = 3 - phase.row - phase.col;
    EXPECT(!phase.participates(out));
    for (bool relay : {false, true}) {
      const auto runs = scripted_phase(n, phase, cfg, 1, relay);
      for (int me = 0; me < n; ++me) {
        const ScriptedRun& run = runs[static_cast<size_t>(me)];
        const PhaseResult& res = run.res;
        const double slow = script_T(std::max(phase.row, phase.col), iters) / 1e3;
        // A rank outside the cell posts and times it only on a transport that
        // routes through it; its time is then its own, and in neither case
        // does it take part in the phase's maximum or in a flow's.
        EXPECT((me == out && !relay) == run.log.empty());
        EXPECT_REL(res.rank_seconds[static_cast<size_t>(phase.row)], script_T(phase.row, iters) / 1e3);
        EXPECT_REL(res.rank_seconds[static_cast<size_t>(phase.col)], script_T(phase.col, iters) / 1e3);
        if (relay)
          EXPECT_REL(res.rank_seconds[static_cast<size_t>(out)], script_T(out, iters) / 1e3);
        else
          EXPECT(res.rank_seconds[static_cast<size_t>(out)] == 0);
        EXPECT_REL(res.seconds_per_iter, slow / iters);
        EXPECT(res.flows.size() == 1);
        if (res.flows.size() != 1) continue;
        EXPECT_REL(res.flows[0].seconds, slow / iters);
        EXPECT_REL(res.agg_gbs, static_cast<double>(cfg.bytes) / (slow / iters) / 1e9);
        EXPECT(res.flows[0].iter_us.n == static_cast<size_t>(iters));
        EXPECT_REL(res.flows[0].iter_us.mean * iters, script_T(phase.col, iters) * 1e3);
      }
    }
  }
  EXPECT(cells == 2 && idle == n);  // (0,1): the rank outside would be the slowest by script; (2,0): the sender is
}

// The host clock is not scripted: sync() on rank r takes at least
// 2 ms * (r + 1), so lower bounds and structure are what can be asserted.
class SlowSync final : public Transport {
 public:
  explicit SlowSync(Transport& t) : t_(&t) {}
  std::string name() const override { return "slow-sync"; }
  int rank() const override { return t_->rank(); }
  int nranks() const override { return t_->nranks(); }
  void* alloc(size_t b) override { return t_->alloc(b); }
  void release(void* p) override { t_->release(p); }
  void fill(void* p, size_t b, uint64_t s) override { t_->fill(p, b, s); }
  void zero(void* p, size_t b) override { t_->zero(p, b); }
  VerifyResult verify(const void* p, size_t b, uint64_t s) override { return t_->verify(p, b, s); }
  void group_begin() override { t_->group_begin(); }
  void send(const void* p, size_t b, int peer) override { t_->send(p, b, peer); }
  void recv(void* p, size_t b, int peer) override { t_->recv(p, b, peer); }
  void group_end() override { t_->group_end(); }
  int mark() override { return t_->mark(); }
  double elapsed_ms(int a, int b) override { return t_->elapsed_ms(a, b); }
  void clear_marks() override { t_->clear_marks(); }
  void sync() override {
    std::this_thread::sleep_for(std::chrono::milliseconds(2 * (rank() + 1)));
    t_->sync();
  }

 private:
  Transport* t_;
};

TEST(test_wallclock_phase_lower_bounds) {
  const int n = 3, iters = 5;
  const Schedule s = make_pair_schedule(n, Direction::Uni);
  const Phase* cell = nullptr;
  for (const Phase& p : s.phases)
    if (p.row == 0 && p.col == 1) cell = &p;
  EXPECT(cell != nullptr);
  if (!cell) return;
  run_ranks(n, [&](Bootstrap& b, Transport& host) {
    SlowSync t(host);
    RunConfig cfg = scripted_config(iters, 0);
    cfg.timing = Timing::Wallclock;
    Buffers bufs(t, cfg.bytes, 1);
    const PhaseResult res = run_phase(t, b, *cell, 0, cfg, bufs);
    // Barrier-bracketed host clock: every rank, the one outside the cell
    // included, waits for the slowest, whose every iteration syncs.
    double most = 0;
    for (double v : res.rank_seconds) {
      EXPECT(v >= iters * 2e-3);
      most = std::max(most, v);
    }
    EXPECT(res.rank_seconds[2] > 0);
    EXPECT_REL(res.seconds_per_iter, most / iters);  // the maximum over ALL ranks
    EXPECT(res.flows.size() == 1);
    for (const FlowResult& f : res.flows) {
      EXPECT_REL(f.seconds, res.seconds_per_iter);  // every flow carries the phase time
      EXPECT_REL(f.gbs, static_cast<double>(cfg.bytes) / f.seconds / 1e9);
      EXPECT(f.iter_us.n == static_cast<size_t>(iters));
      EXPECT(f.iter_us.min >= 2e3 * (f.flow.dst + 1));
      // The receiver's samples lie inside its window.
      EXPECT(f.iter_us.mean * iters <= res.rank_seconds[static_cast<size_t>(f.flow.dst)] * 1e6 * (1 + 1e-12));
    }
    // This rank's wall clock brackets this rank's window (every rank checks
    // its own: clocks of two ranks' barrier exits are not ordered).
    EXPECT(res.wall_seconds >= res.rank_seconds[static_cast<size_t>(b.rank())]);
    b.barrier();
  });
}

TEST(test_scripted_latency) {
  // Host-posted: the leader (lower rank) halves each mark-to-mark interval,
  // the follower contributes nothing, and (a, b) carries rank a's summary.
  const int n = 4, iters = 12;
  run_ranks(n, [&](Bootstrap& b, Transport& host) {
    ScriptedClock t(host);
    Buffers bufs(t, 64, 1);
    const auto lat = run_latency(t, b, 8, iters, 2, bufs);
    EXPECT(lat.size() == 6);
    for (const LatencyResult& l : lat) {
      EXPECT(l.a < l.b && l.method == "host");
      std::vector<double> want;
      for (long i = 0; i < iters; ++i) want.push_back((script_T(l.a, i + 1) - script_T(l.a, i)) * 1e3 / 2);
      expect_summary(l.one_way_us, want);
    }
    // n - 1 rounds; this rank leads against every higher rank and asks for
    // nothing in the rounds it follows.
    EXPECT(t.asked.size() == static_cast<size_t>(iters) * static_cast<size_t>(n - 1 - b.rank()));
    for (const auto& q : t.asked) EXPECT(q.second == q.first + 1);
    b.barrier();
  });
  // One rank: the self exchange is one way already, not halved.
  {
    auto boot = make_local_bootstrap();
    TransportOptions opt;
    opt.timeout_s = 60;
    auto host = make_host_transport(*boot, opt);
    ScriptedClock t(*host);
    Buffers bufs(t, 64, 1);
    const auto lat = run_latency(t, *boot, 8, iters, 2, bufs);
    EXPECT(lat.size() == 1);
    if (lat.size() == 1) {
      EXPECT(lat[0].a == 0 && lat[0].b == 0);
      std::vector<double> want;
      for (long i = 0; i < iters; ++i) want.push_back((script_T(0, i + 1) - script_T(0, i)) * 1e3);
      expect_summary(lat[0].one_way_us, want);
    }
  }
  // Pre-posted behind a (faked) gate in batches of 8: every batch takes
  // marks 0..k, its first exchange (the interval ending at mark 1) is not
  // sampled, and batches overlap by one so exactly `iters` samples remain.
  setenv("P2P_TEST_FAKE_GATE", "1", 1);
  const int total = 37, batch = 8;
  run_ranks(n, [&](Bootstrap& b, Transport& host) {
    ScriptedClock t(host);
    Buffers bufs(t, 64, 1);
    const auto lat = run_latency(t, b, 8, total, 2, bufs, batch);
    EXPECT(lat.size() == 6);
    for (const LatencyResult& l : lat) {
      EXPECT(l.method == "preposted");
      std::vector<double> want;
      for (int left = total; left > 0;) {
        const int k = std::min(batch, left + 1);  // exchanges of this batch; k - 1 of them are sampled
        for (long i = 2; i <= k; ++i) want.push_back((script_T(l.a, i) - script_T(l.a, i - 1)) * 1e3 / 2);
        left -= k - 1;
      }
      EXPECT(want.size() == static_cast<size_t>(total));
      expect_summary(l.one_way_us, want);
    }
    EXPECT(t.asked.size() == static_cast<size_t>(total) * static_cast<size_t>(n - 1 - b.rank()));
    for (const auto& q : t.asked) EXPECT(q.second != 1 && q.second == q.first + 1);
    b.barrier();
  });
  unsetenv("P2P_TEST_FAKE_GATE");
}

TEST(test_scripted_step_driver) {
  // Every rank takes part in every step: step() takes two marks, run_steps
  // one per boundary; a step's time is the interval of its recorded pair.
  run_ranks(4, [&](Bootstrap& b, Transport& host) {
    ScriptedClock t(host);
    const int me = b.rank();
    StepDriver d(t, b, make_tournament_schedule(4, Direction::Bi), 4100, 2, true, 21);
    d.connect();
    d.reset();
    EXPECT(!t.log.empty() && t.log.back() == 'c');
    long m = t.count('m');
    d.step(0);
    EXPECT(t.count('m') == m + 2);
    d.step(1);
    EXPECT(t.count('m') == m + 4);
    d.run_steps(2, 4);
    EXPECT(t.count('m') == m + 4 + 5);
    d.sync();
    t.asked.clear();
    std::vector<double> ms = d.step_ms();
    const std::vector<std::pair<int, int>> pairs{{0, 1}, {2, 3}, {4, 5}, {5, 6}, {6, 7}, {7, 8}};
    EXPECT(t.asked == pairs);
    EXPECT(ms.size() == pairs.size());
    double chained = 0;
    for (size_t k = 0; k < ms.size() && k < pairs.size(); ++k) {
      EXPECT_REL(ms[k], script_T(me, pairs[k].second) - script_T(me, pairs[k].first));
      if (k >= 2) chained += ms[k];
    }
    EXPECT_REL(chained, script_T(me, 8) - script_T(me, 4));  // chained steps tile their run
    EXPECT(d.verify_steps(2, 4).mismatches == 0);
    // reset(): ordinals restart, the next run starts from a fresh mark, and
    // only the new steps are reported.
    d.reset();
    EXPECT(t.log.back() == 'c');
    m = t.count('m');
    d.run_steps(6, 2);
    EXPECT(t.count('m') == m + 3);
    d.sync();
    t.asked.clear();
    ms = d.step_ms();
    const std::vector<std::pair<int, int>> fresh{{0, 1}, {1, 2}};
    EXPECT(t.asked == fresh);
    EXPECT(ms.size() == 2);
    if (ms.size() == 2) {
      EXPECT_REL(ms[0], script_T(me, 1));
      EXPECT_REL(ms[1], script_T(me, 2) - script_T(me, 1));
    }
    b.barrier();
  });
  // The pair schedule on 3 ranks: every rank sits steps out (the diagonal,
  // and the cells of the two others).  Those read 0.0, break the chain, and
  // the step after one starts from a mark of its own.
  run_ranks(3, [&](Bootstrap& b, Transport& host) {
    ScriptedClock t(host);
    const int me = b.rank();
    const Schedule s = make_pair_schedule(3, Direction::Uni);
    const long steps = static_cast<long>(s.phases.size());
    EXPECT(steps == 9);
    StepDriver d(t, b, s, 4100, 2, true, 22);
    d.connect();
    d.reset();
    const long m = t.count('m');
    d.run_steps(0, steps);
    d.sync();
    std::vector<double> want;
    long next = 0, last = -1, sat_out = 0;
    for (long k = 0; k < steps; ++k) {
      if (!s.phases[static_cast<size_t>(k)].participates(me)) {
        want.push_back(0.0);
        last = -1;
        ++sat_out;
        continue;
      }
      const long a = last >= 0 ? last : next++;
      const long z = next++;
      want.push_back(script_T(me, z) - script_T(me, a));
      last = z;
    }
    EXPECT(sat_out == 5);  // 3 diagonal cells and the 2 between the others
    EXPECT(t.count('m') == m + next);
    const std::vector<double> ms = d.step_ms();
    EXPECT(ms.size() == want.size());
    for (size_t k = 0; k < ms.size() && k < want.size(); ++k) {
      if (want[k] == 0.0)
        EXPECT(ms[k] == 0.0);
      else
        EXPECT_REL(ms[k], want[k]);
    }
    EXPECT(d.verify_steps(0, steps).mismatches == 0);
    b.barrier();
  });
}

// remote_slots: the k-th send to a peer meets the k-th receive from it.
TEST(test_remote_slots_repeated_peer) {
  Schedule s = make_ring_schedule(2, Direction::Bi);
  for (const Phase& p : s.phases)
    for (int r = 0; r < 2; ++r) {
      auto rs = remote_slots(p, r);
      EXPECT(rs.size() == p.ranks[static_cast<size_t>(r)].send_to.size());
      std::vector<int> sorted = rs;
      std::sort(sorted.begin(), sorted.end());
      EXPECT(std::unique(sorted.begin(), sorted.end()) == sorted.end());
    }
}

// RCCL INFO-log parsing (csrc/rccl_log.cpp).  The two files are RCCL
// 2.26.6's own logs of a 1-rank communicator on MI355X, default channels and
// NCCL_MAX_P2P_NCHANNELS=1 (WARN lines dropped); the 4-rank connection lines
// follow NCCL's p2p / net / shm formats.
static std::string read_file(const std::string& path) {
  std::ifstream in(path);
  std::stringstream ss;
  ss << in.rdbuf();
  return ss.str();
}

TEST(test_rccl_log_init_block) {
  const std::string dir = P2P_TEST_DATA;
  RcclInitInfo a = parse_rccl_init(read_file(dir + "/rccl_info_self_nch64.txt"));
  EXPECT(a.found() && a.p2p_channels == 64 && a.p2p_per_peer == 128 && a.nranks == 1 && a.nnodes == 1);
  EXPECT(a.unroll == 1);  // "RCCL Unroll Factor (pre-set): 1"
  EXPECT(parse_rccl_init("x NCCL INFO RCCL Unroll Factor (user-defined): 4\n").unroll == 4);
  EXPECT(rccl_op_channels(a, false, 2) == 64);  // 64 x 16 MiB = the 1 GiB limit seen on the self path
  RcclInitInfo b = parse_rccl_init(read_file(dir + "/rccl_info_self_nch1.txt"));
  EXPECT(b.found() && b.p2p_channels == 1 && b.p2p_per_peer == 2);
  EXPECT(rccl_op_channels(b, false, 2) == 1);  // the 16 MiB limit of the repro
  EXPECT(parse_rccl_connections(read_file(dir + "/rccl_info_self_nch64.txt")).empty());
  EXPECT(!parse_rccl_init("no such lines\n").found());
  EXPECT(rccl_op_channels(RcclInitInfo(), false, 2) == 0);
  RcclInitInfo c;
  c.p2p_channels = 64;
  c.p2p_per_peer = 8;
  EXPECT(rccl_op_channels(c, false, 2) == 8 && rccl_op_channels(c, true, 2) == 2 && rccl_op_channels(c, true, 0) == 8);
}

TEST(test_rccl_log_connections) {
  const std::string log =
      "host:1:2 [0] NCCL INFO Channel 00/0 : 1[1] -> 2[2] via P2P/IPC/read\n"
      "host:1:2 [0] NCCL INFO Channel 01/0 : 1[1] -> 2[2] via P2P/IPC/read\n"
      "host:1:2 [0] NCCL INFO Channel 00/0 : 2[2] -> 1[1] via P2P/IPC/read\n"
      "host:1:2 [0] NCCL INFO Channel 00/0 : 1[0] -> 3[0] [send] via NET/Socket/0\n"
      "host:1:2 [0] NCCL INFO Channel 00/0 : 0[0] -> 1[0] [receive] via NET/Socket/0\n"
      "host:1:2 [0] NCCL INFO Channel 02/0 : 0[0] -> 1[0] [receive] via NET/Socket/0\n"
      "host:1:2 [0] NCCL INFO Channel 05 : 1[1] -> 4[4] via SHM/direct/direct\n"
      "host:1:2 [0] NCCL INFO Channel 00/128 : 0\n"
      "garbage Channel x : via\n";
  auto conns = parse_rccl_connections(log);
  EXPECT(conns.size() == 7);
  EXPECT(conns[0].channel == 0 && conns[0].src == 1 && conns[0].dst == 2 && conns[0].via == "P2P/IPC/read");
  EXPECT(conns[3].via == "NET/Socket/0" && conns[6].channel == 5 && conns[6].via == "SHM/direct/direct");
  auto links = rccl_peer_links(conns, 1, 5);
  EXPECT(links.size() == 5);
  // peer 0: receive-side lines only (channels 0 and 2)
  EXPECT(links[0].transport == "NET" && links[0].channels_connected == 2);
  EXPECT(links[4].transport == "SHM" && links[4].channels_connected == 1);
  EXPECT(links[1].transport == "self");
  EXPECT(links[2].transport == "P2P" && links[2].channels_connected == 2 && links[2].via == "P2P/IPC/read");
  EXPECT(links[3].transport == "NET" && links[3].channels_connected == 1);
  auto none = rccl_peer_links({}, 0, 2);
  EXPECT(none[1].transport.empty() && none[1].channels_connected == 0);
}

TEST(test_rccl_log_four_net_ranks) {
  // Rank 1's own log of a 4-rank RCCL 2.26.6 job on one MI355X, every rank a
  // host of its own (P2P_RCCL_DISTINCT_HOSTS: RCCL's socket transport).
  const std::string text = read_file(std::string(P2P_TEST_DATA) + "/rccl_info_4rank_net_rank1.txt");
  RcclInitInfo info = parse_rccl_init(text);
  EXPECT(info.nranks == 4 && info.nnodes == 4 && info.p2p_channels == 4 && info.p2p_per_peer == 2);
  EXPECT(rccl_op_channels(info, true, 2) == 2);
  auto conns = parse_rccl_connections(text);
  EXPECT(conns.size() > 12);
  int p2p = 0;
  for (const auto& c : conns) p2p += c.conn_index == 1;
  EXPECT(p2p == 12);
  auto links = rccl_peer_links(conns, 1, 4);
  for (int p : {0, 2, 3}) {
    EXPECT(links[static_cast<size_t>(p)].transport == "NET");
    EXPECT(links[static_cast<size_t>(p)].via == "NET/Socket/0");
    EXPECT(links[static_cast<size_t>(p)].channels_connected == 2);  // the p2p connections: 2 per net peer
  }
  EXPECT(links[1].transport == "self");
}

TEST(test_rccl_op_limits_from_connection_lines) {
  // a canned log in RCCL 2.26's format (rank 1 of 4 GPUs
  // on one host, two communicators, P2P/IPC connections; one line of another
  // process-local communicator).  Init line: 8 p2p channels per peer.
  const std::string text = read_file(std::string(P2P_TEST_DATA) + "/rccl_info_4rank_p2p_rank1_canned.txt");
  RcclInitInfo info = parse_rccl_init(text);
  EXPECT(info.p2p_channels == 64 && info.p2p_per_peer == 8 && info.nnodes == 1);
  auto all_conns = parse_rccl_connections(text);
  EXPECT(all_conns.size() == 23 && all_conns[0].comm == "0x5a5a0100" && all_conns.back().comm == "0x77770100");
  auto conns = connections_of(all_conns, {"0x5a5a0100", "0x5a5a0900"});
  EXPECT(conns.size() == 22);
  auto links = rccl_peer_links(conns, 1, 4);
  EXPECT(links[0].transport == "P2P" && links[0].channels_connected == 4);  // 4 send channels on both comms
  EXPECT(links[2].transport == "P2P" && links[2].channels_connected == 2);  // 8 on one comm, 2 on the other
  EXPECT(links[3].transport.empty() && links[3].channels_connected == 0);   // only a foreign comm's line
  EXPECT(rccl_peer_links(all_conns, 1, 4)[3].channels_connected == 1);
  const int init = rccl_op_channels(info, false, 2);
  EXPECT(init == 8);
  const std::vector<int> prop = proposed_op_channels({init, 0, init, init}, links, 1);
  EXPECT((prop == std::vector<int>{4, 0, 2, 0}));
  // Every rank's proposals: rank 0 saw 4 towards rank 1, ranks 2 and 3 none.
  std::vector<int> all(16, 0);
  for (int p = 0; p < 4; ++p) all[static_cast<size_t>(4 + p)] = prop[static_cast<size_t>(p)];
  all[0 * 4 + 1] = 4;
  std::vector<std::string> src(4, "init");
  const std::vector<int> agreed = agree_op_channels(all, 4, 1, {2, 64, 2, 2}, &src);
  EXPECT((agreed == std::vector<int>{4, 64, 2, 2}));
  EXPECT(src[0] == "connection lines" && src[2] == "connection lines" && src[1] == "init" && src[3] == "init");
  // The peer's view is the same pair: rank 0 agrees on 4 towards rank 1.
  EXPECT(agree_op_channels(all, 4, 0, {64, 2, 2, 2})[1] == 4);
  // The 4-rank NET log: 2 channels connected per peer, as the init rule said.
  const std::string net = read_file(std::string(P2P_TEST_DATA) + "/rccl_info_4rank_net_rank1.txt");
  auto nl = rccl_peer_links(parse_rccl_connections(net), 1, 4);
  const int ninit = rccl_op_channels(parse_rccl_init(net), true, 2);
  EXPECT((proposed_op_channels({ninit, 0, ninit, ninit}, nl, 1) == std::vector<int>{2, 0, 2, 2}));
}

TEST(test_rccl_unparsed_peers_keep_their_raw_lines) {
  // connection lines in a layout parse_rccl_connections
  // does not know (peer 2 here) leave a connected same-host peer with no
  // channels; rccl_unparsed_peers names it with its raw lines, connection-like
  // lines first.  Peer 1's line is in the known layout.
  const std::string text =
      "node:4711:4711 [0] NCCL INFO comm 0x5a5a0100 rank 0 nRanks 4 nNodes 1 localRanks 4 localRank 0 MNNVL 0\n"
      "node:4711:4711 [0] NCCL INFO 64 coll channels, 0 collnet channels, 0 nvls channels, 64 p2p channels, 8 p2p "
      "channels per peer\n"
      "node:4711:4711 [0] NCCL INFO comm 0x5a5a0100 rank 0 nranks 4 cudaDev 0 busId 2d000 - Init COMPLETE\n"
      "node:4711:4730 [0] NCCL INFO Channel 00/1 : 0[0] -> 1[1] via P2P/IPC comm 0x5a5a0100 nRanks 04\n"
      "node:4711:4731 [0] NCCL INFO peer 2 proxy progress thread started\n"
      "node:4711:4731 [0] NCCL INFO P2P channel 04: rank 0 => peer 2 over xGMI (IPC read) comm 0x5a5a0100\r\n"
      "node:4711:4731 [0] NCCL INFO P2P channel 12: rank 0 => peer 2 over xGMI (IPC read) comm 0x5a5a0100\n"
      "node:4711:4731 [0] NCCL INFO busId 2d000 cudaDev 2 nothing about the peer\n";
  auto links = rccl_peer_links(parse_rccl_connections(text), 0, 4);
  EXPECT(links[1].channels_connected == 1 && links[2].channels_connected == 0 && links[3].channels_connected == 0);
  // Peers 1 and 2 were exchanged with; 3 was not (no connection expected).
  auto u = rccl_unparsed_peers(text, links, {0, 0, 0, 0}, {0, 1, 1, 0}, 0);
  EXPECT(u.size() == 1 && u[0].peer == 2 && u[0].lines.size() == 3);
  if (u.size() == 1 && u[0].lines.size() == 3) {
    EXPECT(u[0].lines[0].find("P2P channel 04: rank 0 => peer 2") != std::string::npos);
    EXPECT(u[0].lines[1].find("channel 12") != std::string::npos && u[0].lines[1].back() != '\r');
    EXPECT(u[0].lines[2].find("proxy progress") != std::string::npos);
  }
  // A peer RCCL reaches over its network transport is judged by the init
  // line, and the line budget holds.
  EXPECT(rccl_unparsed_peers(text, links, {0, 0, 1, 0}, {0, 1, 1, 0}, 0).empty());
  auto capped = rccl_unparsed_peers(text, links, {0, 0, 0, 0}, {0, 1, 1, 0}, 0, 2);
  EXPECT(capped.size() == 1 && capped[0].lines.size() == 2);
  // Every peer parsed: nothing to report.
  const std::string known = read_file(std::string(P2P_TEST_DATA) + "/rccl_info_4rank_p2p_rank1_canned.txt");
  auto kl = rccl_peer_links(connections_of(parse_rccl_connections(known), {"0x5a5a0100", "0x5a5a0900"}), 1, 4);
  EXPECT(rccl_unparsed_peers(known, kl, {0, 0, 0, 0}, {1, 0, 1, 0}, 1).empty());
}

TEST(test_rccl_log_sample) {
  // What a node run keeps of RCCL's real log: version, channel counts, the
  // first connection lines, in that order.
  const std::string text = read_file(std::string(P2P_TEST_DATA) + "/rccl_info_4rank_p2p_rank1_canned.txt");
  auto s = rccl_log_sample(text, 3);
  EXPECT(s.size() == 5);
  if (s.size() == 5) {
    EXPECT(s[0].find("RCCL version : 2.26.6") != std::string::npos);
    EXPECT(s[1].find("8 p2p channels per peer") != std::string::npos);
    // p2p connection lines ("xx/1") before the collectives' ("xx/0").
    EXPECT(s[2].find("Channel 00/1 : 1[1] -> 0[0] via P2P/IPC") != std::string::npos);
    EXPECT(s[4].find("Channel 32/1 : 1[1] -> 0[0]") != std::string::npos);
  }
  EXPECT(rccl_log_sample("", 4).empty());
  // Only collective lines: they fill the sample.
  auto c = rccl_log_sample("x NCCL INFO Channel 00/0 : 3[0] -> 0[0] [receive] via NET/Socket/0 comm 0x1\n", 4);
  EXPECT(c.size() == 1 && c[0].find("via NET/Socket/0") != std::string::npos);
}

// printf of one of RCCL's log formats with the values a run would print: the
// n-th integer conversion (%d, %02d, %x, %lx) takes ints[n] (0 past the end),
// except the last, which takes `last` (nRanks on a connection line); %s takes
// strs[n] ("" past the end); %p takes `comm`.
static std::string expand_rccl_format(const std::string& fmt, const std::vector<long>& ints,
                                      const std::vector<std::string>& strs, long last, const std::string& comm) {
  int total = 0;
  for (size_t i = 0; i + 1 < fmt.size(); ++i)
    if (fmt[i] == '%') {
      size_t j = i + 1;
      while (j < fmt.size() && (std::isdigit(static_cast<unsigned char>(fmt[j])) || fmt[j] == 'l')) ++j;
      total += j < fmt.size() && (fmt[j] == 'd' || fmt[j] == 'x');
      i = j;
    }
  std::string out;
  size_t ni = 0, ns = 0;
  for (size_t i = 0; i < fmt.size(); ++i) {
    if (fmt[i] != '%' || i + 1 >= fmt.size()) {
      out += fmt[i];
      continue;
    }
    size_t j = i + 1;
    const bool zero = fmt[j] == '0';
    int width = 0;
    while (j < fmt.size() && std::isdigit(static_cast<unsigned char>(fmt[j]))) width = width * 10 + (fmt[j++] - '0');
    while (j < fmt.size() && fmt[j] == 'l') ++j;
    const char conv = fmt[j];
    std::string v;
    if (conv == 'd' || conv == 'x') {
      const long x = ni + 1 == static_cast<size_t>(total) ? last : (ni < ints.size() ? ints[ni] : 0);
      ++ni;
      std::ostringstream s;
      if (conv == 'x') s << std::hex;
      s << x;
      v = s.str();
    } else if (conv == 's') {
      v = ns < strs.size() ? strs[ns] : "";
      ++ns;
    } else if (conv == 'p') {
      v = comm;
    }
    if (static_cast<int>(v.size()) < width) v.insert(0, static_cast<size_t>(width) - v.size(), zero ? '0' : ' ');
    out += v;
    i = j;
  }
  return out;
}

TEST(test_rccl_log_formats_of_the_library) {
  // VERDICT r4 missing #2: RCCL's xGMI P2P transport cannot run on one GPU,
  // so the lines a node run prints are pinned from the printf formats
  // compiled into the linked librccl.so (scripts/rccl_formats.py;
  // tests/test_rccl_formats.py checks the file against the library).  Every
  // "Channel" format, expanded with a hex bus id in the brackets, parses to
  // the channel, connection index, ranks, comm and transport class it names;
  // every init format to the counts it carries.
  std::ifstream in(std::string(P2P_TEST_DATA) + "/rccl_2.26.6_log_formats.txt");
  int formats = 0, channel_formats = 0, init_formats = 0;
  std::string ipc_format, counts_format, ranks_format;
  for (std::string fmt; std::getline(in, fmt);) {
    if (fmt.empty() || fmt[0] == '#') continue;
    ++formats;
    const std::string pre = "node:4711:4711 [3] NCCL INFO ";
    if (fmt.find("p2p channels per peer") != std::string::npos) {
      counts_format = fmt;
      RcclInitInfo i = parse_rccl_init(pre + expand_rccl_format(fmt, {64, 0, 0, 64}, {}, 8, ""));
      EXPECT(i.p2p_channels == 64 && i.p2p_per_peer == 8);
      ++init_formats;
      continue;
    }
    if (fmt.find(" nNodes ") != std::string::npos) {
      ranks_format = fmt;
      RcclInitInfo i = parse_rccl_init(pre + expand_rccl_format(fmt, {3, 8, 2, 4, 3}, {}, 0, "0x5a5a0100"));
      EXPECT(i.nranks == 8 && i.nnodes == 2);
      ++init_formats;
      continue;
    }
    if (fmt.find("Unroll Factor") != std::string::npos) {
      EXPECT(parse_rccl_init(pre + expand_rccl_format(fmt, {}, {}, 4, "")).unroll == 4);
      ++init_formats;
      continue;
    }
    const size_t via = fmt.find(" via ");
    const std::string cls = fmt.substr(via + 5, fmt.find('/', via) - via - 5);
    const bool with_conn = fmt.rfind("Channel %02d/", 0) == 0;
    const std::vector<long> ints = with_conn ? std::vector<long>{17, 1, 3, 0x5d000, 6, 0xbd000}
                                             : std::vector<long>{17, 3, 0x5d000, 6, 0xbd000};
    const std::string line = "node:4711:4731 [3] NCCL INFO " +
                             expand_rccl_format(fmt, ints, {"direct", "/read", ""}, 8, "0x5a5a0100");
    auto conns = parse_rccl_connections(line);
    if (fmt.rfind("CollNet", 0) == 0) {  // collnet: no channel connection to a peer
      EXPECT(conns.empty());
      continue;
    }
    ++channel_formats;
    if (fmt.find("via P2P/IPC") != std::string::npos) ipc_format = fmt;
    EXPECT(conns.size() == 1);
    if (conns.size() != 1) {
      std::fprintf(stderr, "  not parsed: %s\n", line.c_str());
      continue;
    }
    const RcclConnection& c = conns[0];
    EXPECT(c.channel == 17 && c.conn_index == (with_conn ? 1 : 0) && c.src == 3 && c.dst == 6);
    EXPECT(c.comm == "0x5a5a0100" && c.via.rfind(cls + "/", 0) == 0);
    auto links = rccl_peer_links(conns, 3, 8);
    EXPECT(links[6].transport == (cls == "COLLNET" ? "NET" : cls) && links[6].channels_connected == 1);
  }
  EXPECT(formats == 14 && channel_formats == 8 && init_formats == 4);
  if (ipc_format.empty() || counts_format.empty() || ranks_format.empty()) return;
  // Rank 3 of 8 on one node, in the library's formats: 8 p2p channels per
  // peer on send lines, 2 ring channels ("/0") towards each neighbour.
  std::string text = "node:4711:4711 [3] NCCL INFO " +
                     expand_rccl_format(ranks_format, {3, 8, 1, 8, 3}, {}, 0, "0x5a5a0100") + "\n" +
                     "node:4711:4711 [3] NCCL INFO " + expand_rccl_format(counts_format, {64, 0, 0, 64}, {}, 8, "") +
                     "\n";
  for (int p : {2, 4})
    for (int ch = 0; ch < 2; ++ch)
      text += "node:4711:4730 [3] NCCL INFO " +
              expand_rccl_format(ipc_format, {ch, 0, 3, 0x5d000, p, 0x1d000 + 0x20000L * p}, {"/read"}, 8,
                                 "0x5a5a0100") +
              "\n";
  for (int p = 0; p < 8; ++p)
    for (int k = 0; p != 3 && k < 8; ++k)
      text += "node:4711:4731 [3] NCCL INFO " +
              expand_rccl_format(ipc_format, {p + 8 * k, 1, 3, 0x5d000, p, 0x1d000 + 0x20000L * p}, {"/read"}, 8,
                                 "0x5a5a0100") +
              "\n";
  auto links = rccl_peer_links(parse_rccl_connections(text), 3, 8);
  for (int p = 0; p < 8; ++p) {
    if (p == 3) continue;
    EXPECT(links[static_cast<size_t>(p)].transport == "P2P" && links[static_cast<size_t>(p)].channels_connected == 8);
    EXPECT(links[static_cast<size_t>(p)].via == "P2P/IPC/read");
  }
  const int init = rccl_op_channels(parse_rccl_init(text), false, 2);
  EXPECT(init == 8);
  EXPECT((proposed_op_channels(std::vector<int>(8, init), links, 3) == std::vector<int>{8, 8, 8, 0, 8, 8, 8, 8}));
  std::vector<char> touched(8, 1);
  touched[3] = 0;
  EXPECT(rccl_unparsed_peers(text, links, std::vector<char>(8, 0), touched, 3).empty());
}

TEST(test_rccl_log_warnings_and_env_ownership) {
  // The private log's WARN extraction (the text RCCL errors carry) on a file
  // this test owns: NCCL_DEBUG_FILE set by the user is read as it is.
  const std::string path = "/tmp/p2p_host_test_rccl_log_" + std::to_string(static_cast<int>(getpid())) + ".txt";
  {
    std::ofstream f(path);
    for (int i = 0; i < 6; ++i) f << "x NCCL WARN problem " << i << "\nx NCCL INFO fine\n";
  }
  setenv("NCCL_DEBUG_FILE", path.c_str(), 1);
  EXPECT(rccl_log_file().path == path && !rccl_log_file().ours);
  const std::string w = rccl_log_warnings(0);
  EXPECT(w.find("problem 2") != std::string::npos && w.find("problem 5") != std::string::npos &&
         w.find("problem 1") == std::string::npos && w.find("fine") == std::string::npos);
  EXPECT(rccl_log_size() > 0 && rccl_log_since(rccl_log_size()).empty());
  unsetenv("NCCL_DEBUG_FILE");
  std::remove(path.c_str());
}

TEST(test_link_transport_mismatch) {
  EXPECT(link_transport_mismatch("XGMI/1", "SHM"));
  EXPECT(link_transport_mismatch("XGMI/1", "NET"));
  EXPECT(!link_transport_mismatch("XGMI/1", "P2P"));
  EXPECT(!link_transport_mismatch("XGMI/1", ""));  // not connected / no log: nothing to judge
  EXPECT(!link_transport_mismatch("XGMI/2", "SHM"));  // no direct link
  EXPECT(!link_transport_mismatch("PCIE/2", "SHM"));
  EXPECT(!link_transport_mismatch("same-gpu", "NET"));
  EXPECT(!link_transport_mismatch("n/a", "NET"));
}

TEST(test_fabric_findings_cli) {
  // The CLI's fabric check (report.cpp fabric_findings): alike links pass;
  // one slow cell, or a pair whose both directions together are below a uni
  // cell, are named.  GB/s per direction, row = sender.
  const int n = 3;
  std::vector<double> uni = {0, 50, 51, 49, 0, 50, 50, 52, 0};
  std::vector<double> bi = {0, 45, 46, 44, 0, 45, 45, 47, 0};
  EXPECT(fabric_findings(uni, &bi, n).empty());
  EXPECT(fabric_findings(uni, nullptr, n).empty());
  std::vector<double> slow = uni;
  slow[2 * n + 1] = 12.0;
  auto f = fabric_findings(slow, &bi, n);
  EXPECT(f.size() == 1 && f[0].find("cell 2->1 12.00") != std::string::npos);
  std::vector<double> weak_bi = bi;
  weak_bi[0 * n + 1] = 20.0;
  weak_bi[1 * n + 0] = 20.0;  // 40 both ways < 50 and < 49
  f = fabric_findings(uni, &weak_bi, n);
  EXPECT(f.size() == 2 && f[0].find("pair 0<->1 both directions 40.00") != std::string::npos);
  // Unmeasured cells (0) are not judged.
  std::vector<double> partial = {0, 50, 0, 0, 0, 0, 0, 0, 0};
  EXPECT(fabric_findings(partial, nullptr, n).empty());
}

TEST(test_abort_if_idle_waits_for_native_calls) {
  // the watchdog aborts the communicators itself only when no
  // engine call is open, then takes no more calls.  (Closes the engine for
  // the rest of this process: the last test.)
  int ran = 0;
  push_abort_hook([&ran](int) { ++ran; });
  // a hook that blocks (ncclCommAbort on a kernel that never
  // exits) must not hold the engine's lock: a thread entering meanwhile is
  // refused at once instead of queueing behind the abort.
  std::atomic<bool> in_hook{false}, release{false};
  push_abort_hook([&](int) {
    in_hook = true;
    for (int i = 0; i < 10000 && !release; ++i) std::this_thread::sleep_for(std::chrono::milliseconds(1));
  });
  {
    NativeCall in_engine;
    EXPECT(!abort_if_idle() && ran == 0 && !abort_done());
  }
  std::atomic<bool> aborted{false};
  std::thread watchdog([&] { aborted = abort_if_idle(); });
  for (int i = 0; i < 5000 && !in_hook; ++i) std::this_thread::sleep_for(std::chrono::milliseconds(1));
  EXPECT(in_hook && !aborted);
  const auto t0 = std::chrono::steady_clock::now();
  bool entered = true;
  {
    NativeCall probe(std::nothrow);
    entered = probe.entered();
  }
  const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  EXPECT(!entered && waited < 0.5);
  release = true;
  watchdog.join();
  EXPECT(aborted && ran == 1 && abort_done());
  set_throw_on_fatal(true);
  bool refused = false;
  try {
    NativeCall late;
  } catch (const Error& e) {
    refused = std::string(e.what()).find("aborted") != std::string::npos;
  }
  set_throw_on_fatal(false);
  EXPECT(refused);
  EXPECT(abort_if_idle() && ran == 1);  // the hooks ran once
}

// ------------------- push / relay rendezvous: recorded programs vs a model ----
//
// T0r.  The IPC push and relay engines promise that no byte is written into a
// receive slot before its receiver said it is ready, and that a receive
// completes on the stream only once every writer's bytes are there.  Which
// flags a rank posts and waits for, with which values, in which order around
// its copies, is decided by PushPlanner (push_plan.hpp).  Here the real runner
// drives one planner per rank, exactly as IpcTransport does, over the host
// transport (which moves the bytes, so the runner's own verification runs);
// what each rank would have put on its stream is recorded as a program, and
// the N programs are evaluated in a model written from the contract:
//   * a flag belongs to (owner rank, kind, posting rank) and only grows;
//   * a rank's stream runs its program in order; the host posts it in order,
//     sync() waits for the stream, a collective of the control plane (barrier,
//     all-gather) orders what every rank's host knew before it against what
//     any rank posts after it;
//   * a signal issues all its posts, then waits for all its waits;
//   * a wait (flag, v) is enabled by the first post that brings the flag to
//     >= v, and learns from it: only that the post was issued, unless the
//     post's signal released first -- then everything that happened before
//     the signal on the poster's stream.
// Happens-before is tracked with two prefixes per rank: `strong[r] = k`, the
// first k operations of r's program have completed and are visible, and
// `weak[r] = k`, the signals among them have issued their posts.
//
// Deliberately not a property: a relay reads the sender's send buffer without
// telling the sender when it is finished (a writer raises `done` at the
// receiver only).  The runner rewrites send regions only between barriers, so
// the model does not ask for an edge from a relay's copy back to the sender.

struct RvOp {
  enum Kind { Signal, Copy, Sync, Collective } kind = Signal;
  long group = -1;  // rank-local group the operation belongs to (Signal, Copy)
  // Signal
  std::vector<PushFlag> posts, waits;
  bool release_first = false;
  bool after_copies = false;
  // Copy
  PushCopy copy;
  long seq = -1;  // which message (src, dst, slot) of the run it belongs to
};

struct RvRecv {  // a message as its receiver posted it
  long group = -1;
  int src = -1, slot = 0;
  size_t bytes = 0, src_offset = 0;
  long seq = -1;
  bool payload = true;  // false: posted under an injected skip fault (every rank's, in these tests)
};

struct RvProgram {
  std::vector<RvOp> ops;
  std::vector<RvRecv> recvs;
};

class RendezvousRecorder final : public Transport {
 public:
  RendezvousRecorder(Transport& t, bool relay, int max_signals)
      : t_(&t), plan_(t.rank(), t.nranks(), relay, RouteOptions(), max_signals) {}
  std::string name() const override { return "rendezvous-recorder"; }
  int rank() const override { return t_->rank(); }
  int nranks() const override { return t_->nranks(); }
  void* alloc(size_t b) override { return t_->alloc(b); }
  void release(void* p) override { t_->release(p); }
  void fill(void* p, size_t b, uint64_t s) override { t_->fill(p, b, s); }
  void zero(void* p, size_t b) override { t_->zero(p, b); }
  VerifyResult verify(const void* p, size_t b, uint64_t s) override { return t_->verify(p, b, s); }
  int mark() override { return t_->mark(); }
  double elapsed_ms(int a, int b) override { return t_->elapsed_ms(a, b); }
  void clear_marks() override { t_->clear_marks(); }
  void register_buffers(const BufferSet& set) override {
    sets_.push_back(set);
    t_->register_buffers(set);
  }
  void unregister_buffers(void* send) override {
    sets_.erase(std::remove_if(sets_.begin(), sets_.end(), [&](const BufferSet& s) { return s.send == send; }), sets_.end());
    t_->unregister_buffers(send);
  }
  void sync() override {
    t_->sync();
    RvOp op;
    op.kind = RvOp::Sync;
    prog.ops.push_back(op);
  }
  void note_collective() {
    RvOp op;
    op.kind = RvOp::Collective;
    prog.ops.push_back(op);
  }

  void group_begin() override {
    EXPECT(!in_group_);
    in_group_ = true;
    plan_.group_begin();
    t_->group_begin();
  }
  bool wants_group_flows() const override { return plan_.relay(); }
  void group_flows(const void*, const std::vector<GroupFlow>& flows, size_t bytes) override {
    EXPECT(in_group_);
    for (const auto& f : flows)
      if (f.src != f.dst) message(f.src, f.dst, f.slot);
    for (const PushCopy& c : plan_.group_flows(flows, bytes, discarding())) add_copy(c);
  }
  void send(const void* p, size_t b, int peer) override { send_to_slot(p, b, peer, 0); }
  void send_to_slot(const void* p, size_t bytes, int peer, int slot) override {
    const BufferSet* set = nullptr;
    for (const auto& s : sets_)
      if (p >= s.send && static_cast<const char*>(p) + bytes <= static_cast<const char*>(s.send) + s.send_bytes) set = &s;
    EXPECT(set != nullptr);
    if (!set) return;
    message(rank(), peer, slot);
    PushCopy c;
    if (plan_.send(static_cast<size_t>(static_cast<const char*>(p) - static_cast<const char*>(set->send)), bytes, peer, slot,
                   discarding(), &c))
      add_copy(c);
    t_->send(p, bytes, peer);
    if (!in_group_) flush();
  }
  void recv(void* p, size_t b, int peer) override { recv_from(p, b, peer, 0); }
  void recv_from(void* p, size_t bytes, int peer, size_t src_offset) override {
    int slot = -1;
    for (const auto& s : sets_) {
      const char* base = static_cast<const char*>(s.recv);
      const char* q = static_cast<const char*>(p);
      if (q >= base && q < base + s.stride * static_cast<size_t>(s.nslots) && static_cast<size_t>(q - base) % s.stride == 0)
        slot = static_cast<int>(static_cast<size_t>(q - base) / s.stride);
    }
    EXPECT(slot >= 0);
    if (slot < 0) return;
    prog.recvs.push_back({group_, peer, slot, bytes, src_offset, message(peer, rank(), slot), !discarding()});
    plan_.recv(peer, slot);
    t_->recv(p, bytes, peer);
    if (!in_group_) flush();
  }
  void group_end() override {
    EXPECT(in_group_);
    in_group_ = false;
    EXPECT(plan_.group_complete());
    flush();
    t_->group_end();
  }

  RvProgram prog;

 private:
  // The ordinal of the message (src, dst, slot) among those this rank has
  // seen between the two ranks and that slot; one message per group and key,
  // whichever of group_flows / send / recv names it first.
  long message(int src, int dst, int slot) {
    const std::array<int, 3> key{src, dst, slot};
    auto it = in_group_seq_.find(key);
    if (it != in_group_seq_.end()) return it->second;
    const long seq = count_[key]++;
    in_group_seq_[key] = seq;
    return seq;
  }
  void add_copy(const PushCopy& c) {
    RvOp op;
    op.kind = RvOp::Copy;
    op.copy = c;
    op.seq = message(c.src, c.dst, c.slot);
    copies_.push_back(op);
  }
  // What IpcTransport::flush_push puts on the stream, in its order.
  void flush() {
    const PushFlush f = plan_.flush();
    auto signals = [&](const std::vector<PushPiece>& pieces, bool after) {
      for (const PushPiece& piece : pieces) {
        RvOp op;
        op.kind = RvOp::Signal;
        op.group = group_;
        op.posts = piece.posts;
        op.waits = piece.waits;
        op.release_first = piece.release_first;
        op.after_copies = after;
        prog.ops.push_back(op);
      }
    };
    signals(f.pre, false);
    for (RvOp& c : copies_) {
      c.group = group_;
      prog.ops.push_back(c);
    }
    signals(f.post, true);
    copies_.clear();
    in_group_seq_.clear();
    ++group_;
  }

  Transport* t_;
  PushPlanner plan_;
  std::vector<BufferSet> sets_;
  bool in_group_ = false;
  long group_ = 0;
  std::vector<RvOp> copies_;
  std::map<std::array<int, 3>, long> count_, in_group_seq_;
};

// The control plane with its collectives noted in the rank's program.
class CollectiveRecorder final : public Bootstrap {
 public:
  CollectiveRecorder(Bootstrap& b, RendezvousRecorder& rec) : b_(&b), rec_(&rec) {}
  int rank() const override { return b_->rank(); }
  int size() const override { return b_->size(); }
  void allgather(const void* mine, void* all, size_t bytes) override {
    rec_->note_collective();
    b_->allgather(mine, all, bytes);
  }
  void bcast(void* buf, size_t bytes, int root) override { b_->bcast(buf, bytes, root); }
  void barrier() override {
    rec_->note_collective();
    b_->barrier();
  }
  void abort(int code) override { b_->abort(code); }
  std::string name() const override { return b_->name(); }
  void set_timeout(double s) override { b_->set_timeout(s); }

 private:
  Bootstrap* b_;
  RendezvousRecorder* rec_;
};

struct RvClock {
  std::vector<long> strong, weak;
  explicit RvClock(int n = 0) : strong(static_cast<size_t>(n), 0), weak(static_cast<size_t>(n), 0) {}
  void join(const RvClock& o) {
    for (size_t i = 0; i < strong.size(); ++i) {
      strong[i] = std::max(strong[i], o.strong[i]);
      weak[i] = std::max(weak[i], o.weak[i]);
    }
  }
};

// Evaluates the programs; returns what the contract forbids, one line each
// ("liveness: ...", "ready: ...", "done: ...", "reuse: ...", "tiling: ...",
// "balance: ...", "monotone: ...").
static std::vector<std::string> rendezvous_violations(const std::vector<RvProgram>& progs) {
  std::vector<std::string> bad;
  const int n = static_cast<int>(progs.size());
  struct Post {
    unsigned long long value;
    RvClock carried;
  };
  std::map<std::array<int, 3>, std::vector<Post>> flags;         // (owner, kind, poster) -> posts in order
  std::map<std::array<int, 3>, unsigned long long> most_waited;  // the same key -> highest value waited for
  struct Rank {
    size_t hp = 0, sp = 0;   // next operation of the host / of the stream
    bool posted = false;     // the signal at sp has issued its posts
    RvClock host, stream;
    std::vector<RvClock> posted_at;  // per operation: what the host knew when it posted it
    std::vector<RvClock> at;         // per operation: Copy: when it ran; Signal: when it ended
  };
  std::vector<Rank> st(static_cast<size_t>(n));
  for (int r = 0; r < n; ++r) {
    Rank& k = st[static_cast<size_t>(r)];
    k.host = k.stream = RvClock(n);
    k.posted_at.assign(progs[static_cast<size_t>(r)].ops.size(), RvClock());
    k.at.assign(progs[static_cast<size_t>(r)].ops.size(), RvClock());
  }
  auto on_stream = [](const RvOp& op) { return op.kind == RvOp::Signal || op.kind == RvOp::Copy; };
  for (bool progress = true; progress;) {
    progress = false;
    for (int r = 0; r < n; ++r) {
      Rank& k = st[static_cast<size_t>(r)];
      const auto& ops = progs[static_cast<size_t>(r)].ops;
      // The host: posts stream work without waiting, waits at a sync.
      while (k.hp < ops.size()) {
        const RvOp& op = ops[k.hp];
        if (on_stream(op)) {
          k.posted_at[k.hp] = k.host;
        } else if (op.kind == RvOp::Sync) {
          if (k.sp < k.hp) break;
          k.host.join(k.stream);
        } else {
          break;  // a collective: below, once every rank is at one
        }
        ++k.hp;
        progress = true;
      }
      // The stream: what was posted, in order.
      while (k.sp < k.hp) {
        const RvOp& op = ops[k.sp];
        const size_t i = k.sp;
        if (!on_stream(op)) {
          ++k.sp;
          progress = true;
          continue;
        }
        if (op.kind == RvOp::Copy) {
          k.stream.join(k.posted_at[i]);
          k.at[i] = k.stream;
        } else {
          if (!k.posted) {
            k.stream.join(k.posted_at[i]);
            RvClock carried(n);
            if (op.release_first) carried = k.stream;
            carried.weak[static_cast<size_t>(r)] = static_cast<long>(i) + 1;
            for (const PushFlag& f : op.posts) {
              auto& line = flags[{f.peer, f.kind, r}];
              if (!line.empty() && line.back().value >= f.value)
                bad.push_back(strfmt("monotone: rank %d posts %llu on a flag that holds %llu", r, f.value, line.back().value));
              line.push_back({f.value, carried});
            }
            k.posted = true;
            progress = true;
          }
          bool open = true;
          for (const PushFlag& f : op.waits) {
            const auto& line = flags[{r, f.kind, f.peer}];
            open = open && !line.empty() && line.back().value >= f.value;
          }
          if (!open) break;
          for (const PushFlag& f : op.waits) {
            const auto& line = flags[{r, f.kind, f.peer}];
            for (const Post& p : line)
              if (p.value >= f.value) {
                k.stream.join(p.carried);
                break;
              }
            auto& w = most_waited[{r, f.kind, f.peer}];
            w = std::max(w, f.value);
          }
          k.posted = false;
          k.stream.weak[static_cast<size_t>(r)] = static_cast<long>(i) + 1;
          k.at[i] = k.stream;
        }
        k.stream.strong[static_cast<size_t>(r)] = static_cast<long>(i) + 1;
        if (op.kind == RvOp::Signal) k.at[i].strong[static_cast<size_t>(r)] = static_cast<long>(i) + 1;
        ++k.sp;
        progress = true;
      }
    }
    // A collective completes once every rank's host has reached it.
    bool all = true;
    for (int r = 0; r < n; ++r) {
      const Rank& k = st[static_cast<size_t>(r)];
      const auto& ops = progs[static_cast<size_t>(r)].ops;
      all = all && k.hp < ops.size() && ops[k.hp].kind == RvOp::Collective;
    }
    if (all) {
      RvClock joined(n);
      for (const Rank& k : st) joined.join(k.host);
      for (Rank& k : st) {
        k.host = joined;
        ++k.hp;
      }
      progress = true;
    }
  }
  for (int r = 0; r < n; ++r) {
    const Rank& k = st[static_cast<size_t>(r)];
    const auto& ops = progs[static_cast<size_t>(r)].ops;
    if (k.hp == ops.size() && k.sp == ops.size()) continue;
    std::string what = k.sp < ops.size() && ops[k.sp].kind == RvOp::Signal ? "a signal that waits for" : "operation";
    if (k.sp < ops.size() && ops[k.sp].kind == RvOp::Signal)
      for (const PushFlag& f : ops[k.sp].waits) what += strfmt(" (%d,%s,%llu)", f.peer, f.kind == kPushReady ? "ready" : "done", f.value);
    bad.push_back(strfmt("liveness: rank %d stops at %zu of %zu (host at %zu): %s", r, k.sp, ops.size(), k.hp, what.c_str()));
  }
  if (!bad.empty()) return bad;  // the orders below are those of a finished run

  // Balance: what was posted last on a flag is what was last waited for.
  for (const auto& kv : flags)
    if (!kv.second.empty() && kv.second.back().value != most_waited[kv.first])
      bad.push_back(strfmt("balance: flag (%d,%d,%d) was posted up to %llu and waited for up to %llu", kv.first[0], kv.first[1],
                           kv.first[2], kv.second.back().value, most_waited[kv.first]));
  for (const auto& kv : most_waited)
    if (flags[kv.first].empty()) bad.push_back(strfmt("balance: flag (%d,%d,%d) is waited for and never posted", kv.first[0], kv.first[1], kv.first[2]));

  // Every copy, by the message it belongs to.
  struct Written {
    int writer;
    size_t index;
    const RvOp* op;
  };
  std::map<std::array<long, 4>, std::vector<Written>> by_message;  // (src, dst, slot, seq)
  size_t ncopies = 0;
  for (int w = 0; w < n; ++w) {
    const auto& ops = progs[static_cast<size_t>(w)].ops;
    for (size_t i = 0; i < ops.size(); ++i)
      if (ops[i].kind == RvOp::Copy) {
        by_message[{ops[i].copy.src, ops[i].copy.dst, ops[i].copy.slot, ops[i].seq}].push_back({w, i, &ops[i]});
        ++ncopies;
      }
  }
  size_t matched = 0;
  struct Landed {
    long order;  // position of the message in the receiver's posting order
    Written w;
  };
  std::map<std::array<int, 2>, std::vector<Landed>> by_slot;  // (dst, slot)
  for (int d = 0; d < n; ++d) {
    const RvProgram& prog = progs[static_cast<size_t>(d)];
    for (size_t m = 0; m < prog.recvs.size(); ++m) {
      const RvRecv& rv = prog.recvs[m];
      auto found = by_message.find({rv.src, d, rv.slot, rv.seq});
      std::vector<Written> parts = found == by_message.end() ? std::vector<Written>() : found->second;
      matched += parts.size();
      if (!rv.payload) {
        if (!parts.empty()) bad.push_back(strfmt("tiling: %zu copies of a discarded message %d->%d", parts.size(), rv.src, d));
        continue;
      }
      // Tiling: the parts cover [0, bytes) once, each from the same offset of
      // the sender's message.
      std::sort(parts.begin(), parts.end(), [](const Written& a, const Written& b) { return a.op->copy.offset < b.op->copy.offset; });
      size_t end = 0;
      bool tiles = true;
      for (const Written& p : parts) {
        tiles = tiles && p.op->copy.offset == end && p.op->copy.src_offset == rv.src_offset && p.op->copy.bytes > 0;
        end += p.op->copy.bytes;
      }
      if (!tiles || end != rv.bytes)
        bad.push_back(strfmt("tiling: message %d->%d slot %d #%ld of %zu bytes is covered up to %zu by %zu copies", rv.src, d,
                             rv.slot, rv.seq, rv.bytes, end, parts.size()));
      // The receiver's two signals of the group.
      long last_post = -1;
      for (size_t i = 0; i < prog.ops.size(); ++i)
        if (prog.ops[i].kind == RvOp::Signal && prog.ops[i].group == rv.group && prog.ops[i].after_copies)
          last_post = static_cast<long>(i);
      for (const Written& p : parts) {
        by_slot[{d, rv.slot}].push_back({static_cast<long>(m), p});
        if (p.writer == d) {  // a self message: stream order, no rendezvous
          if (p.op->group != rv.group) bad.push_back(strfmt("ready: self copy of rank %d outside its receive's group", d));
          continue;
        }
        // Writer waits for ready: the copy knows of the receiver's signal
        // that tells this writer so.
        long ready_at = -1;
        for (size_t i = 0; i < prog.ops.size(); ++i) {
          const RvOp& op = prog.ops[i];
          if (op.kind != RvOp::Signal || op.group != rv.group || op.after_copies) continue;
          for (const PushFlag& f : op.posts)
            if (f.peer == p.writer && f.kind == kPushReady) ready_at = static_cast<long>(i);
        }
        const RvClock& when = st[static_cast<size_t>(p.writer)].at[p.index];
        if (ready_at < 0 || when.weak[static_cast<size_t>(d)] < ready_at + 1)
          bad.push_back(strfmt("ready: rank %d writes %d->%d slot %d #%ld before rank %d said it is ready", p.writer, rv.src, d,
                               rv.slot, rv.seq, d));
        // Receive completes after the data: the end of the receiver's
        // post-signal knows the copy, which only a releasing done gives it.
        if (last_post < 0 || st[static_cast<size_t>(d)].at[static_cast<size_t>(last_post)].strong[static_cast<size_t>(p.writer)] <
                                 static_cast<long>(p.index) + 1)
          bad.push_back(strfmt("done: rank %d's receive of %d->%d slot %d #%ld completes without rank %d's copy", d, rv.src, d,
                               rv.slot, rv.seq, p.writer));
      }
    }
  }
  if (matched != ncopies) bad.push_back(strfmt("tiling: %zu of %zu copies belong to no posted receive", ncopies - matched, ncopies));
  // Slot reuse: copies into overlapping bytes of one slot are ordered like
  // the receiver posted their messages.
  for (const auto& kv : by_slot) {
    const auto& v = kv.second;
    for (size_t a = 0; a < v.size(); ++a)
      for (size_t b = 0; b < v.size(); ++b) {
        if (v[a].order >= v[b].order) continue;
        const PushCopy &x = v[a].w.op->copy, &y = v[b].w.op->copy;
        if (x.offset + x.bytes <= y.offset || y.offset + y.bytes <= x.offset) continue;
        const RvClock& later = st[static_cast<size_t>(v[b].w.writer)].at[v[b].w.index];
        if (later.strong[static_cast<size_t>(v[a].w.writer)] < static_cast<long>(v[a].w.index) + 1)
          bad.push_back(strfmt("reuse: slot %d of rank %d: rank %d's copy and rank %d's later one are unordered", kv.first[1],
                               kv.first[0], v[a].w.writer, v[b].w.writer));
      }
  }
  return bad;
}

static void expect_no_violations(const std::vector<std::string>& bad, const char* what) {
  EXPECT(bad.empty());
  for (size_t i = 0; i < bad.size() && i < 5; ++i) std::fprintf(stderr, "  %s: %s\n", what, bad[i].c_str());
}

static size_t relayed_copies(const std::vector<RvProgram>& progs) {
  size_t k = 0;
  for (size_t w = 0; w < progs.size(); ++w)
    for (const RvOp& op : progs[w].ops)
      k += op.kind == RvOp::Copy && op.copy.src != static_cast<int>(w) && op.copy.dst != static_cast<int>(w);
  return k;
}

// One recorded session of `n` ranks: the planner in push or relay mode, the
// caller's body over the recording transport and control plane.
static std::vector<RvProgram> record_rendezvous(int n, bool relay, int max_signals,
                                                const std::function<void(Bootstrap&, RendezvousRecorder&)>& body) {
  std::vector<RvProgram> progs(static_cast<size_t>(n));
  run_ranks(n, [&](Bootstrap& b, Transport& host) {
    RendezvousRecorder t(host, relay, max_signals);
    CollectiveRecorder boot(b, t);
    body(boot, t);
    boot.barrier();
    progs[static_cast<size_t>(b.rank())] = t.prog;
  });
  return progs;
}

static uint64_t record_schedules(Bootstrap& b, Transport& t, int n, size_t bytes) {
  uint64_t bad = 0;
  for (Mode m : {Mode::Pair, Mode::Ring, Mode::AllPairs, Mode::Tournament, Mode::Self})
    for (Direction d : {Direction::Uni, Direction::Bi}) {
      Schedule s = make_schedule(m, d, n);
      RunConfig cfg;
      cfg.bytes = bytes;
      cfg.iters = 2;
      cfg.warmup = 1;
      cfg.verify = true;
      Buffers bufs(t, cfg.bytes, std::max(1, s.max_recv_slots()));
      for (auto& ph : run_schedule(t, b, s, cfg, bufs)) bad += ph.total_mismatches;
    }
  return bad;
}

TEST(test_rendezvous_schedules_against_model) {
  for (int max_signals : {kPushMaxSignals, 2})
    for (bool relay : {false, true})
      for (int n : {2, 3, 4, 8}) {
        std::atomic<uint64_t> mism{0};
        const auto progs = record_rendezvous(n, relay, max_signals, [&](Bootstrap& b, RendezvousRecorder& t) {
          mism += record_schedules(b, t, n, 8192);
        });
        EXPECT(mism == 0);
        expect_no_violations(rendezvous_violations(progs), relay ? "relay 8K" : "push 8K");
        if (!relay) EXPECT(relayed_copies(progs) == 0);
      }
}

TEST(test_rendezvous_relayed_stripes_against_model) {
  // 4 MiB messages: above RouteOptions::min_bytes, so stripes go through ranks
  // that are neither the sender nor the receiver.
  for (int max_signals : {kPushMaxSignals, 2})
    for (int n : {3, 4}) {
      std::atomic<uint64_t> mism{0};
      const auto progs = record_rendezvous(n, true, max_signals, [&](Bootstrap& b, RendezvousRecorder& t) {
        mism += record_schedules(b, t, n, size_t{4} << 20);
      });
      EXPECT(mism == 0);
      EXPECT(relayed_copies(progs) > 0);
      expect_no_violations(rendezvous_violations(progs), "relay 4M");
    }
  // Eight ranks: a tournament round's pairs share the relays (two segments
  // per link), a single pair has six.
  for (int max_signals : {kPushMaxSignals, 2}) {
    std::atomic<uint64_t> mism{0};
    const auto progs = record_rendezvous(8, true, max_signals, [&](Bootstrap& b, RendezvousRecorder& t) {
      RunConfig cfg;
      cfg.bytes = size_t{4} << 20;
      cfg.iters = 2;
      cfg.warmup = 1;
      cfg.verify = true;
      Schedule s = make_schedule(Mode::Tournament, Direction::Bi, 8);
      s.phases.resize(2);
      Buffers bufs(t, cfg.bytes, s.max_recv_slots());
      for (auto& ph : run_schedule(t, b, s, cfg, bufs)) mism += ph.total_mismatches;
      Schedule p = make_schedule(Mode::Pair, Direction::Uni, 8);
      restrict_cells(&p, {{0, 1}, {5, 2}}, true);
      for (auto& ph : run_schedule(t, b, p, cfg, bufs)) mism += ph.total_mismatches;
    });
    EXPECT(mism == 0);
    EXPECT(relayed_copies(progs) > 0);
    expect_no_violations(rendezvous_violations(progs), "relay 4M x8");
  }
}

// Steps posted back to back: depth 2 over 5 steps of a one-phase schedule
// reuses every slot (generations 0 1 0 1 0) with no barrier and no host sync
// in between; the tournament's phases change the flows from step to step.
static std::vector<RvProgram> record_steps(bool relay, int max_signals, size_t bytes, std::atomic<uint64_t>* mism) {
  const int n = 4;
  return record_rendezvous(n, relay, max_signals, [&](Bootstrap& b, RendezvousRecorder& t) {
    for (int which = 0; which < 2; ++which) {
      StepOptions so;
      so.depth = 2;
      so.batch = which == 1;
      StepDriver d(t, b, which == 0 ? make_ring_schedule(n, Direction::Bi) : make_tournament_schedule(n, Direction::Bi), bytes,
                   3, true, 21 + static_cast<uint64_t>(which), so);
      EXPECT(d.depth() == 2);
      d.connect();
      d.poison();
      d.run_steps(0, 5);
      d.sync();
      *mism += d.verify_steps(0, 5).mismatches;
    }
  });
}

TEST(test_rendezvous_step_driver_against_model) {
  for (int max_signals : {kPushMaxSignals, 2})
    for (bool relay : {false, true})
      for (size_t bytes : {size_t{8192}, size_t{2} << 20}) {
        if (!relay && bytes > 8192) continue;
        std::atomic<uint64_t> mism{0};
        const auto progs = record_steps(relay, max_signals, bytes, &mism);
        EXPECT(mism == 0);
        EXPECT((relayed_copies(progs) > 0) == (relay && bytes > 8192));
        expect_no_violations(rendezvous_violations(progs), "steps");
      }
}

TEST(test_rendezvous_fuzz_against_model) {
  // Random groups: self messages, repeated pairs (several messages share one
  // flag of a group), sizes on both sides of the relay threshold.
  for (int max_signals : {kPushMaxSignals, 2})
    for (bool relay : {false, true}) {
      std::atomic<uint64_t> mism{0};
      const auto progs = record_rendezvous(4, relay, max_signals, [&](Bootstrap& b, RendezvousRecorder& t) {
        mism += fuzz_transport(t, b, 40, 0x5EED, size_t{2} << 20);
      });
      EXPECT(mism == 0);
      if (relay) EXPECT(relayed_copies(progs) > 0);
      expect_no_violations(rendezvous_violations(progs), "fuzz");
    }
}

TEST(test_rendezvous_discard_still_runs_the_protocol) {
  // An injected skip fault moves no payload; every flag is still posted and
  // waited for, so no peer hangs and the counters stay in step for the
  // groups that follow.
  for (bool relay : {false, true}) {
    const int n = 4;
    const Phase phase = make_tournament_schedule(n, Direction::Bi).phases[1];
    const size_t bytes = size_t{2} << 20;
    auto run = [&](bool discard_only) {
      return record_rendezvous(n, relay, kPushMaxSignals, [&](Bootstrap& b, RendezvousRecorder& t) {
        Buffers bufs(t, bytes, phase.max_recv_slots());
        t.set_discard(true);
        for (int i = 0; i < 3; ++i) post_phase_iteration(t, phase, bytes, bufs);
        t.set_discard(false);
        if (!discard_only)
          for (int i = 0; i < 2; ++i) post_phase_iteration(t, phase, bytes, bufs);
        t.sync();
        b.barrier();
      });
    };
    const auto none = run(true);
    size_t signals = 0;
    for (const auto& p : none)
      for (const RvOp& op : p.ops) signals += op.kind == RvOp::Signal;
    EXPECT(signals == 2u * 3 * n);  // a pre and a post signal per group and rank
    expect_no_violations(rendezvous_violations(none), "discard");
    // Copies again once the fault is lifted, on flags that went on counting.
    expect_no_violations(rendezvous_violations(run(false)), "discard, then payload");
  }
}

// The model has teeth: each of these changes to a recorded set of programs
// breaks the contract, and the model must say so.
TEST(test_rendezvous_model_rejects_mutations) {
  for (bool relay : {false, true}) {
    std::atomic<uint64_t> mism{0};
    const auto good = record_steps(relay, kPushMaxSignals, relay ? size_t{2} << 20 : size_t{8192}, &mism);
    EXPECT(mism == 0 && rendezvous_violations(good).empty());
    auto has = [](const std::vector<std::string>& bad, const char* what) {
      for (const auto& s : bad)
        if (s.rfind(what, 0) == 0) return true;
      return false;
    };
    // The first copy to another rank, in a group that follows another group
    // to the same receiver, and the signals around it.
    int w = -1;
    size_t ci = 0, pre = 0, post = 0;
    for (int r = 0; r < static_cast<int>(good.size()) && w < 0; ++r) {
      const auto& ops = good[static_cast<size_t>(r)].ops;
      for (size_t i = 0; i < ops.size() && w < 0; ++i) {
        if (ops[i].kind != RvOp::Copy || ops[i].copy.dst == r) continue;
        const int d = ops[i].copy.dst;
        long a = -1, z = -1;
        for (size_t j = 0; j < ops.size(); ++j) {
          if (ops[j].kind != RvOp::Signal || ops[j].group != ops[i].group) continue;
          for (const PushFlag& f : ops[j].waits)
            if (!ops[j].after_copies && f.peer == d && f.kind == kPushReady && f.value >= 2) a = static_cast<long>(j);
          for (const PushFlag& f : ops[j].posts)
            if (ops[j].after_copies && f.peer == d && f.kind == kPushDone) z = static_cast<long>(j);
        }
        if (a < 0 || z < 0) continue;
        w = r, ci = i, pre = static_cast<size_t>(a), post = static_cast<size_t>(z);
      }
    }
    EXPECT(w >= 0);
    if (w < 0) continue;
    const int d = good[static_cast<size_t>(w)].ops[ci].copy.dst;
    auto drop = [](std::vector<PushFlag>* v, int peer) {
      v->erase(std::remove_if(v->begin(), v->end(), [&](const PushFlag& f) { return f.peer == peer; }), v->end());
    };
    {  // drop one ready wait
      auto m = good;
      drop(&m[static_cast<size_t>(w)].ops[pre].waits, d);
      EXPECT(has(rendezvous_violations(m), "ready:"));
    }
    {  // drop one done wait: the receiver's, for this writer, in the copy's group
      auto m = good;
      bool dropped = false;
      const RvOp& c = good[static_cast<size_t>(w)].ops[ci];
      long group = -1;
      for (const RvRecv& rv : good[static_cast<size_t>(d)].recvs)
        if (rv.src == c.copy.src && rv.slot == c.copy.slot && rv.seq == c.seq) group = rv.group;
      for (RvOp& op : m[static_cast<size_t>(d)].ops)
        if (op.kind == RvOp::Signal && op.group == group && op.after_copies) {
          const size_t before = op.waits.size();
          drop(&op.waits, w);
          dropped = dropped || op.waits.size() < before;
        }
      EXPECT(dropped);
      EXPECT(has(rendezvous_violations(m), "done:"));
    }
    {  // a wait one lower than it must be: the previous group's ready opens it
      auto m = good;
      for (PushFlag& f : m[static_cast<size_t>(w)].ops[pre].waits)
        if (f.peer == d) --f.value;
      EXPECT(has(rendezvous_violations(m), "ready:"));
    }
    {  // the done post in front of its copy
      auto m = good;
      auto& ops = m[static_cast<size_t>(w)].ops;
      size_t first = ci;
      while (first > 0 && ops[first - 1].kind == RvOp::Copy) --first;
      const RvOp moved = ops[post];
      ops.erase(ops.begin() + static_cast<long>(post));
      ops.insert(ops.begin() + static_cast<long>(first), moved);
      EXPECT(has(rendezvous_violations(m), "done:"));
    }
    {  // a done piece that does not release first
      auto m = good;
      m[static_cast<size_t>(w)].ops[post].release_first = false;
      EXPECT(has(rendezvous_violations(m), "done:"));
    }
  }
}

// The planner's pieces on their own: one entry per flag with the highest
// value, at most max_signals posts and waits per piece, every post out before
// or with the first wait, and a release in front of every done post.
TEST(test_push_planner_pieces) {
  std::vector<PushFlag> posts, waits;
  for (int p = 0; p < 5; ++p) posts.push_back({p, kPushDone, static_cast<unsigned long long>(p + 1)});
  posts.push_back({1, kPushDone, 9});  // a second message to rank 1: same flag, higher value
  for (int p = 0; p < 3; ++p) waits.push_back({p, kPushDone, 4});
  const auto one = PushPlanner::pieces(posts, waits, kPushMaxSignals, true);
  EXPECT(one.size() == 1 && one[0].posts.size() == 5 && one[0].waits.size() == 3 && one[0].release_first);
  EXPECT(one[0].posts[1].peer == 1 && one[0].posts[1].value == 9);
  const auto cut = PushPlanner::pieces(posts, waits, 2, true);
  EXPECT(cut.size() == 4);  // posts 2 + 2 + 1, waits 0 + 0 + 2 + 1
  bool waited = false;
  for (const auto& piece : cut) {
    EXPECT(piece.posts.size() <= 2 && piece.waits.size() <= 2);
    EXPECT(piece.posts.empty() || piece.release_first);  // the overflow pieces carry done posts too
    waited = waited || !piece.waits.empty();
    if (waited && &piece != &cut[2]) EXPECT(piece.posts.empty());
  }
  EXPECT(cut.back().release_first);
  for (const auto& piece : PushPlanner::pieces(posts, waits, 2, false)) EXPECT(!piece.release_first);
  EXPECT(PushPlanner::pieces({}, {}, 2, true).empty());
}

// ------------------------- IpcBlocks: the exporting allocator and its pool ----
//
// The IPC transport's block policy (ipc_blocks.hpp) over counting fakes: the
// fake allocator hands out 1, 2, 3, ... as pointers and keeps the live set,
// the fake export writes the pointer into the handle.
namespace {
struct FakeIpcMemory {
  int allocs = 0, frees = 0, exports = 0;
  int fail_allocs = 0;     // the next so many allocations fail
  int refuse_exports = 0;  // the next so many exports are refused
  std::set<void*> live;
  std::vector<std::string> log;            // "alloc <n>", "free <n>", in order
  std::vector<std::pair<size_t, size_t>> refusals;  // what the callback reported
  std::vector<size_t> sizes;               // of every allocation that succeeded

  static void* ptr(int k) { return reinterpret_cast<void*>(static_cast<uintptr_t>(k)); }
  static int num(void* p) { return static_cast<int>(reinterpret_cast<uintptr_t>(p)); }
  static uintptr_t handle_value(const IpcHandle& h) {
    uintptr_t v = 0;
    std::memcpy(&v, h.bytes, sizeof(v));
    return v;
  }

  IpcBlocks blocks(size_t cap, bool size_fix = true) {
    return IpcBlocks(
        cap, size_fix,
        [this](void** p, size_t size) -> const char* {
          if (fail_allocs > 0) {
            --fail_allocs;
            log.push_back("alloc failed");
            return "out of memory";
          }
          *p = ptr(++allocs);
          live.insert(*p);
          sizes.push_back(size);
          log.push_back("alloc " + std::to_string(allocs));
          return nullptr;
        },
        [this](void* p) {
          ++frees;
          EXPECT(live.erase(p) == 1);  // freed once, and only what was allocated
          log.push_back("free " + std::to_string(num(p)));
        },
        [this](void* p, IpcHandle* h) -> const char* {
          ++exports;
          if (refuse_exports > 0) {
            --refuse_exports;
            return "invalid argument";
          }
          const uintptr_t v = reinterpret_cast<uintptr_t>(p);
          std::memset(h->bytes, 0, sizeof(h->bytes));
          std::memcpy(h->bytes, &v, sizeof(v));
          return nullptr;
        },
        [this](size_t blocks, size_t size) { refusals.emplace_back(blocks, size); });
  }
};

template <class F>
std::string fatal_text(F&& f) {
  set_throw_on_fatal(true);
  std::string what;
  try {
    f();
  } catch (const Error& e) {
    what = e.what();
    if (what.empty()) what = "?";
  }
  set_throw_on_fatal(false);
  return what;
}
bool has_text(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }
}  // namespace

TEST(test_ipc_blocks_size_rule) {
  constexpr size_t M = size_t{1} << 20, G = size_t{1} << 30;
  const std::vector<std::array<size_t, 3>> cases = {
      // request, with the fix, without it
      {1, 2 * M, 2 * M},
      {2 * M + 1, 4 * M, 4 * M},
      {2 * G, 4 * G, 2 * G},
      {2 * G - 2 * M, 2 * G - 2 * M, 2 * G - 2 * M},
      {3 * G + 768 * M, 4 * G, 3 * G + 768 * M},
      {4 * G, 4 * G, 4 * G},
      {4 * G + 2 * M, 4 * G + 2 * M, 4 * G + 2 * M},
      {5 * G, 5 * G, 5 * G},
      {7 * G, 8 * G, 7 * G},
  };
  for (const auto& c : cases) {
    EXPECT(IpcBlocks::size_for(c[0], true) == c[1]);
    EXPECT(IpcBlocks::size_for(c[0], false) == c[2]);
  }
  // alloc() asks the allocator for exactly that size, fix on and off.
  FakeIpcMemory on, off;
  IpcBlocks a = on.blocks(0, true), b = off.blocks(0, false);
  a.release(a.alloc(2 * G));
  b.release(b.alloc(2 * G));
  EXPECT(on.sizes == std::vector<size_t>{4 * G} && off.sizes == std::vector<size_t>{2 * G});
  EXPECT(on.live.empty() && off.live.empty());
}

TEST(test_ipc_blocks_pool_reuse_and_cap) {
  constexpr size_t M = size_t{1} << 20;
  {
    FakeIpcMemory mem;
    IpcBlocks blocks = mem.blocks(size_t{64} * M);
    void* p = blocks.alloc(3 * M);  // rounds to 4 MiB
    const uintptr_t h = FakeIpcMemory::handle_value(blocks.handle_of(p));
    EXPECT(h == reinterpret_cast<uintptr_t>(p) && mem.allocs == 1 && mem.exports == 1);
    blocks.release(p);
    EXPECT(mem.frees == 0 && blocks.pooled_bytes() == 4 * M);
    void* q = blocks.alloc(4 * M);  // the same rounded size: the pooled block, no allocate call
    EXPECT(q == p && FakeIpcMemory::handle_value(blocks.handle_of(q)) == h);
    EXPECT(mem.allocs == 1 && mem.exports == 1 && blocks.pooled_bytes() == 0);
    blocks.release(q);
    void* r = blocks.alloc(5 * M);  // another size allocates; the pool keeps its block
    EXPECT(r != p && mem.allocs == 2 && mem.sizes.back() == 6 * M && blocks.pooled_bytes() == 4 * M);
    blocks.release(nullptr);  // a no-op
    blocks.release(r);
    EXPECT(blocks.pooled_bytes() == 10 * M && mem.frees == 0);
    blocks.drain();  // exactly the pooled blocks
    EXPECT(mem.frees == 2 && mem.live.empty() && blocks.pooled_bytes() == 0);
  }
  {
    FakeIpcMemory mem;  // cap 0 keeps nothing
    IpcBlocks blocks = mem.blocks(0);
    void* p = blocks.alloc(1);
    blocks.release(p);
    EXPECT(mem.frees == 1 && mem.live.empty() && blocks.pooled_bytes() == 0);
  }
  {
    FakeIpcMemory mem;  // a release that would pass the cap frees that block
    IpcBlocks blocks = mem.blocks(5 * M);
    void* a = blocks.alloc(2 * M);
    void* b = blocks.alloc(2 * M);
    void* c = blocks.alloc(2 * M);
    blocks.release(a);
    blocks.release(b);
    EXPECT(blocks.pooled_bytes() == 4 * M && mem.frees == 0);
    blocks.release(c);
    EXPECT(blocks.pooled_bytes() == 4 * M && mem.frees == 1 && mem.live.count(c) == 0);
    void* live = blocks.alloc(2 * M);  // from the pool; stays live across the drain
    blocks.drain();
    EXPECT(mem.frees == 2 && mem.live == std::set<void*>{live});
    EXPECT(FakeIpcMemory::handle_value(blocks.handle_of(live)) == reinterpret_cast<uintptr_t>(live));
    blocks.release(live);
    blocks.drain();
    EXPECT(mem.live.empty());
  }
}

TEST(test_ipc_blocks_allocation_failure) {
  constexpr size_t M = size_t{1} << 20;
  {
    FakeIpcMemory mem;  // a pool to give back: drained, then one retry
    IpcBlocks blocks = mem.blocks(size_t{64} * M);
    blocks.release(blocks.alloc(2 * M));
    mem.log.clear();
    mem.fail_allocs = 1;
    void* p = blocks.alloc(4 * M);
    EXPECT((mem.log == std::vector<std::string>{"alloc failed", "free 1", "alloc 2"}));
    EXPECT(p == FakeIpcMemory::ptr(2) && blocks.pooled_bytes() == 0 && mem.live == std::set<void*>{p});
    blocks.release(p);
    mem.log.clear();
    mem.fail_allocs = 2;  // the retry fails too: fatal, and no third attempt
    const std::string what = fatal_text([&] { blocks.alloc(8 * M); });
    EXPECT(has_text(what, "device allocation of 8388608 bytes failed: out of memory"));
    EXPECT((mem.log == std::vector<std::string>{"alloc failed", "free 2", "alloc failed"}));
    EXPECT(mem.live.empty() && mem.fail_allocs == 0);
  }
  {
    FakeIpcMemory mem;  // an empty pool: fatal at once
    IpcBlocks blocks = mem.blocks(size_t{64} * M);
    mem.fail_allocs = 1;
    const std::string what = fatal_text([&] { blocks.alloc(1); });
    EXPECT(has_text(what, "device allocation of 2097152 bytes failed"));
    EXPECT((mem.log == std::vector<std::string>{"alloc failed"}) && mem.live.empty());
  }
}

TEST(test_ipc_blocks_export_refusals) {
  constexpr size_t M = size_t{1} << 20;
  for (int k : {1, 2, 7}) {
    FakeIpcMemory mem;
    IpcBlocks blocks = mem.blocks(0);
    mem.refuse_exports = k;
    void* p = blocks.alloc(2 * M);
    // The (k+1)th block; the k refused ones are held until it exists.
    EXPECT(p == FakeIpcMemory::ptr(k + 1) && mem.allocs == k + 1 && mem.exports == k + 1);
    std::vector<std::string> want;
    for (int i = 1; i <= k + 1; ++i) want.push_back("alloc " + std::to_string(i));
    for (int i = 1; i <= k; ++i) want.push_back("free " + std::to_string(i));
    EXPECT(mem.log == want);
    EXPECT((mem.refusals == std::vector<std::pair<size_t, size_t>>{{static_cast<size_t>(k), 2 * M}}));
    EXPECT(mem.live == std::set<void*>{p});
    EXPECT(FakeIpcMemory::handle_value(blocks.handle_of(p)) == reinterpret_cast<uintptr_t>(p));
    blocks.release(p);
    EXPECT(mem.live.empty());
  }
  {
    FakeIpcMemory mem;  // the eighth refusal in a row is fatal; everything held is freed
    IpcBlocks blocks = mem.blocks(0);
    mem.refuse_exports = 8;
    const std::string what = fatal_text([&] { blocks.alloc(2 * M); });
    EXPECT(has_text(what, "hipIpcGetMemHandle refused 8 fresh 2097152-byte blocks: invalid argument"));
    EXPECT(mem.allocs == 8 && mem.frees == 8 && mem.live.empty() && mem.refusals.empty());
  }
  {
    FakeIpcMemory mem;  // the signal pages' path: another allocator, the same retry, no live-map entry
    IpcBlocks blocks = mem.blocks(0);
    mem.refuse_exports = 2;
    int page_allocs = 0;
    IpcHandle h{};
    void* p = blocks.exportable(4096, &h, [&](void** q, size_t size) -> const char* {
      EXPECT(size == 4096);
      *q = FakeIpcMemory::ptr(100 + ++page_allocs);
      mem.live.insert(*q);
      return nullptr;
    });
    EXPECT(p == FakeIpcMemory::ptr(103) && page_allocs == 3 && mem.frees == 2 && mem.allocs == 0);
    EXPECT((mem.refusals == std::vector<std::pair<size_t, size_t>>{{2, 4096}}) && mem.live == std::set<void*>{p});
    EXPECT(FakeIpcMemory::handle_value(h) == 103);
    EXPECT(has_text(fatal_text([&] { blocks.handle_of(p); }), "exports only buffers it allocated"));
  }
}

TEST(test_ipc_blocks_unknown_pointers) {
  FakeIpcMemory mem;
  IpcBlocks blocks = mem.blocks(size_t{1} << 30);
  void* p = blocks.alloc(1);
  void* stranger = FakeIpcMemory::ptr(999);
  EXPECT(has_text(fatal_text([&] { blocks.release(stranger); }), "release of a buffer this transport did not allocate"));
  EXPECT(has_text(fatal_text([&] { blocks.handle_of(stranger); }), "ipc transport exports only buffers it allocated"));
  blocks.release(p);
  // A pooled block is not a live one: no handle, no second release.
  EXPECT(has_text(fatal_text([&] { blocks.handle_of(p); }), "exports only buffers it allocated"));
  EXPECT(has_text(fatal_text([&] { blocks.release(p); }), "did not allocate"));
  EXPECT(mem.frees == 0 && blocks.pooled_bytes() == (size_t{2} << 20));
  blocks.drain();
  EXPECT(mem.frees == 1 && mem.live.empty());
}

// ------------------------- T0d: the device stream between kernel and report ----
//
// The kernel of the device-initiated stream has its own GPU tests.  What lies
// between it and the numbers a user reads is host code: run_device_stream
// (who sends to whom, which call a cell's numbers come from), StreamPlanner
// (whose page, which slot and line, which sequence base) and
// fold_stream_stamps (what the raw stamps mean).  Three tests:
//   b  run_device_stream over a transport whose device_stream() is scripted:
//      exact expected calls and cell values;
//   a  the calls recorded there, planned by one StreamPlanner per rank and
//      executed by a model of the kernel's protocol over fake pages;
//   c  the fold over scripted stamps in a guarded scratch image.

namespace {

struct StreamCall {
  int send_to, recv_from;
  size_t bytes;
  int iters;
  bool check_all;
  bool operator==(const StreamCall& o) const {
    return send_to == o.send_to && recv_from == o.recv_from && bytes == o.bytes && iters == o.iters && check_all == o.check_all;
  }
};

// What rank `rank` gets back from a call: a pure function of the rank and
// the arguments, injective in them (the key), exact in a double, irregular.
// A value taken from another rank, from the verification call instead of the
// timed one, or from another size therefore differs.
Transport::DeviceStreamTimes stream_script(int rank, const StreamCall& c, bool zero_spans = false) {
  uint64_t key = static_cast<uint64_t>(rank);
  key = key * 9 + static_cast<uint64_t>(c.send_to + 1);
  key = key * 9 + static_cast<uint64_t>(c.recv_from + 1);
  key = key * 2 + (c.check_all ? 1 : 0);
  key = key * 512 + c.bytes / 16;
  key = key * 512 + static_cast<uint64_t>(c.iters);
  const double unit = 1.0 / static_cast<double>(uint64_t{1} << 36);
  Transport::DeviceStreamTimes t;
  t.sent = c.send_to >= 0;
  t.received = c.recv_from >= 0;
  if (t.sent) {
    t.send_span_s = zero_spans ? 0.0 : static_cast<double>(3 * key + 1) * unit;
    for (int i = 0; i < c.iters; ++i)
      t.gap_us.push_back(static_cast<double>(1 + (key + 5 * static_cast<uint64_t>(i)) % 7 + static_cast<uint64_t>(i % 3)) / 8.0);
  }
  if (t.received) {
    // One message has no span between a first and a last arrival.
    t.recv_span_s = zero_spans || c.iters == 1 ? 0.0 : static_cast<double>(5 * key + 2) * unit;
    t.checked_vectors = 7 + key % 100003;
  }
  return t;
}

// The host transport with a scripted device stream; `log` notes stream_setup
// (S), the device_stream calls (v: check_all, t: timed) and, through
// StreamCollectives, the barriers (b) and allgathers (a), in order.
class ScriptedStream final : public Transport {
 public:
  explicit ScriptedStream(Transport& t, bool zero_spans = false) : t_(&t), zero_(zero_spans) {}
  std::string name() const override { return "scripted-stream"; }
  int rank() const override { return t_->rank(); }
  int nranks() const override { return t_->nranks(); }
  void* alloc(size_t b) override { return t_->alloc(b); }
  void release(void* p) override { t_->release(p); }
  void fill(void* p, size_t b, uint64_t s) override { t_->fill(p, b, s); }
  void zero(void* p, size_t b) override { t_->zero(p, b); }
  VerifyResult verify(const void* p, size_t b, uint64_t s) override { return t_->verify(p, b, s); }
  void group_begin() override { t_->group_begin(); }
  void send(const void* p, size_t b, int peer) override { t_->send(p, b, peer); }
  void recv(void* p, size_t b, int peer) override { t_->recv(p, b, peer); }
  void group_end() override { t_->group_end(); }
  int mark() override { return t_->mark(); }
  double elapsed_ms(int a, int b) override { return t_->elapsed_ms(a, b); }
  void clear_marks() override { t_->clear_marks(); }
  void sync() override { t_->sync(); }
  bool supports_device_stream() const override { return true; }
  void stream_setup(int channels, int depth, size_t max_bytes) override {
    setups.push_back({static_cast<size_t>(channels), static_cast<size_t>(depth), max_bytes});
    log += 'S';
  }
  DeviceStreamTimes device_stream(int send_to, int recv_from, size_t bytes, int iters, bool check_all) override {
    const StreamCall c{send_to, recv_from, bytes, iters, check_all};
    calls.push_back(c);
    log += check_all ? 'v' : 't';
    return stream_script(rank(), c, zero_);
  }

  std::string log;
  std::vector<std::array<size_t, 3>> setups;  // (channels, depth, max_bytes)
  std::vector<StreamCall> calls;

 private:
  Transport* t_;
  bool zero_;
};

class StreamCollectives final : public Bootstrap {
 public:
  StreamCollectives(Bootstrap& b, std::string* log) : b_(&b), log_(log) {}
  int rank() const override { return b_->rank(); }
  int size() const override { return b_->size(); }
  void allgather(const void* mine, void* all, size_t bytes) override {
    *log_ += 'a';
    b_->allgather(mine, all, bytes);
  }
  void bcast(void* buf, size_t bytes, int root) override { b_->bcast(buf, bytes, root); }
  void barrier() override {
    *log_ += 'b';
    b_->barrier();
  }
  void abort(int code) override { b_->abort(code); }
  std::string name() const override { return b_->name(); }
  void set_timeout(double s) override { b_->set_timeout(s); }

 private:
  Bootstrap* b_;
  std::string* log_;
};

struct StreamRun {  // one rank's
  std::vector<StreamResult> res;
  std::string log;
  std::vector<std::array<size_t, 3>> setups;
  std::vector<StreamCall> calls;
};

std::vector<StreamRun> scripted_stream(int n, const std::vector<size_t>& sizes, int depth, int channels, int iters,
                                       const std::vector<Direction>& dirs, bool zero_spans = false) {
  std::vector<StreamRun> out(static_cast<size_t>(n));
  run_ranks(n, [&](Bootstrap& b, Transport& host) {
    ScriptedStream t(host, zero_spans);
    StreamCollectives cb(b, &t.log);
    StreamRun& r = out[static_cast<size_t>(b.rank())];
    r.res = run_device_stream(t, cb, sizes, depth, channels, iters, dirs);
    r.log = t.log;
    r.setups = t.setups;
    r.calls = t.calls;
    b.barrier();
  });
  return out;
}

// What the contract of run_device_stream (runner.hpp) makes every rank do,
// from round_robin_rounds alone: its calls, and its log.
void expected_stream_calls(int n, const std::vector<size_t>& sent_sizes, int iters, const std::vector<Direction>& dirs,
                           std::vector<std::vector<StreamCall>>* calls, std::vector<std::string>* logs) {
  calls->assign(static_cast<size_t>(n), {});
  logs->assign(static_cast<size_t>(n), "S");
  const int viters = std::min(iters, 256);
  // One phase: to[r] / from[r] are rank r's peers, -1 for none.
  auto phase = [&](const std::vector<int>& to, const std::vector<int>& from, size_t bytes) {
    for (int r = 0; r < n; ++r) {
      const size_t k = static_cast<size_t>(r);
      const bool active = to[k] >= 0 || from[k] >= 0;
      if (active) {
        (*calls)[k].push_back({to[k], from[k], bytes, viters, true});
        (*calls)[k].push_back({to[k], from[k], bytes, iters, false});
      }
      (*logs)[k] += active ? "bvbta" : "bba";
    }
  };
  if (n == 1) {
    for (size_t di = 0; di < dirs.size(); ++di)
      for (size_t b : sent_sizes) phase({0}, {0}, b);
    return;
  }
  for (const auto& round : round_robin_rounds(n))
    for (Direction d : dirs)
      for (size_t b : sent_sizes) {
        std::vector<int> none(static_cast<size_t>(n), -1), first_to = none, second_to = none, both = none;
        for (const auto& pr : round) {
          first_to[static_cast<size_t>(pr.first)] = pr.second;   // the first member sends
          second_to[static_cast<size_t>(pr.second)] = pr.first;  // the second member sends
          both[static_cast<size_t>(pr.first)] = pr.second;
          both[static_cast<size_t>(pr.second)] = pr.first;
        }
        if (d == Direction::Bi) {
          phase(both, both, b);
        } else {
          // Sender's `to` is the receiver's `from`: first -> second, then back.
          std::vector<int> second_from = none, first_from = none;
          for (const auto& pr : round) {
            second_from[static_cast<size_t>(pr.second)] = pr.first;
            first_from[static_cast<size_t>(pr.first)] = pr.second;
          }
          phase(first_to, second_from, b);
          phase(second_to, first_from, b);
        }
      }
}

bool finite_and_zero(double v) { return std::isfinite(v) && v == 0.0; }

// One scripted run checked from end to end.
void check_scripted_stream(int n, const std::vector<size_t>& sizes, const std::vector<size_t>& sent_sizes, int depth,
                           int channels, int iters, const std::vector<Direction>& dirs, bool zero_spans = false) {
  const auto runs = scripted_stream(n, sizes, depth, channels, iters, dirs, zero_spans);
  std::vector<std::vector<StreamCall>> want_calls;
  std::vector<std::string> want_logs;
  expected_stream_calls(n, sent_sizes, iters, dirs, &want_calls, &want_logs);
  const int viters = std::min(iters, 256);
  auto collectives = [](const std::string& log) {
    std::string o;
    for (char c : log)
      if (c == 'a' || c == 'b') o += c;
    return o;
  };
  for (int me = 0; me < n; ++me) {
    const StreamRun& run = runs[static_cast<size_t>(me)];
    // Setup: once, with the largest rounded size.
    EXPECT(run.setups.size() == 1);
    if (run.setups.size() == 1)
      EXPECT((run.setups[0] == std::array<size_t, 3>{static_cast<size_t>(channels), static_cast<size_t>(depth),
                                                    *std::max_element(sent_sizes.begin(), sent_sizes.end())}));
    // Call order: the same collectives on every rank, the bye rank included;
    // a verification call and a timed call per phase, between their barriers.
    EXPECT(run.log == want_logs[static_cast<size_t>(me)]);
    EXPECT(collectives(run.log) == collectives(runs[0].log));
    EXPECT(run.calls == want_calls[static_cast<size_t>(me)]);

    // Result shape.
    EXPECT(run.res.size() == dirs.size() * sizes.size());
    if (run.res.size() != dirs.size() * sizes.size()) continue;
    std::vector<std::pair<int, int>> pairs;
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < n; ++b)
        if (n == 1 || a != b) pairs.emplace_back(a, b);  // ascending (src, dst)
    for (size_t di = 0; di < dirs.size(); ++di)
      for (size_t si = 0; si < sizes.size(); ++si) {
        const StreamResult& r = run.res[di * sizes.size() + si];
        const bool bi = dirs[di] == Direction::Bi;
        const size_t bytes = sent_sizes[si];
        EXPECT(r.form == (bi ? "bi" : "uni") && r.bytes == bytes);
        EXPECT(r.depth == depth && r.channels == channels && r.iters == iters && r.verify_iters == viters && r.nranks == n);
        EXPECT(r.cells.size() == pairs.size());
        if (r.cells.size() != pairs.size()) continue;
        for (size_t k = 0; k < pairs.size(); ++k) {
          const StreamCell& c = r.cells[k];
          const int src = pairs[k].first, dst = pairs[k].second;
          EXPECT(c.src == src && c.dst == dst);
          // The sender's and the receiver's calls of this cell's phase.
          const bool both = bi || n == 1;
          const StreamCall s_timed{dst, both ? dst : -1, bytes, iters, false};
          const StreamCall r_timed{both ? src : -1, src, bytes, iters, false};
          const StreamCall r_verify{both ? src : -1, src, bytes, viters, true};
          const auto ts = stream_script(src, s_timed, zero_spans);
          const auto tr = stream_script(dst, r_timed, zero_spans);
          const auto vr = stream_script(dst, r_verify, zero_spans);
          EXPECT(c.span_s == ts.send_span_s);
          EXPECT(c.wall_s >= 0);
          expect_summary(c.gap_us, ts.gap_us);
          EXPECT(c.gap_us.n == static_cast<size_t>(iters));
          EXPECT(c.recv_span_s == tr.recv_span_s);
          EXPECT(c.checked_vectors == vr.checked_vectors);
          EXPECT(c.wrong_vectors == 0);
          // runner.hpp: channels x iters messages over the sender's span,
          // channels x (iters - 1) over the receiver's.
          const double msgs = static_cast<double>(channels) * iters;
          if (ts.send_span_s > 0) {
            EXPECT_REL(c.gbs, msgs * static_cast<double>(bytes) / ts.send_span_s / 1e9);
            EXPECT_REL(c.mmsgs, msgs / ts.send_span_s / 1e6);
            EXPECT(c.gbs > 0 && c.mmsgs > 0);
          } else {
            EXPECT(zero_spans && finite_and_zero(c.gbs) && finite_and_zero(c.mmsgs));
          }
          if (tr.recv_span_s > 0) {
            EXPECT_REL(c.recv_gbs, static_cast<double>(channels) * (iters - 1) * static_cast<double>(bytes) / tr.recv_span_s / 1e9);
            EXPECT(c.recv_gbs > 0);
          } else {
            EXPECT((zero_spans || iters == 1) && finite_and_zero(c.recv_gbs));
          }
        }
      }
  }
}

}  // namespace

TEST(test_scripted_device_stream) {
  const std::vector<size_t> sizes{16, 100, 4096}, sent{16, 112, 4096};
  const std::vector<std::vector<Direction>> forms{{Direction::Uni}, {Direction::Bi}, {Direction::Uni, Direction::Bi}};
  // The scripted values differ between a cell's sender and receiver and
  // between the verification and the timed call, or nothing below could tell
  // them apart.
  {
    const StreamCall timed{1, 1, 112, 300, false}, verify{1, 1, 112, 256, true};
    EXPECT(stream_script(0, timed).send_span_s != stream_script(1, {0, 0, 112, 300, false}).send_span_s);
    EXPECT(stream_script(0, timed).recv_span_s != stream_script(0, verify).recv_span_s);
    EXPECT(stream_script(0, timed).checked_vectors != stream_script(0, verify).checked_vectors);
    EXPECT(stream_script(0, timed).send_span_s != stream_script(0, timed).recv_span_s);
  }
  for (int n : {1, 2, 3, 4, 5})
    for (const auto& dirs : forms)
      for (int iters : {1, 3, 300}) check_scripted_stream(n, sizes, sent, n % 2 ? 8 : 3, 1 + n % 3, iters, dirs);
  // The largest size is itself rounded; a zero span leaves zero rates.
  check_scripted_stream(3, {100, 16}, {112, 16}, 8, 2, 20, forms[2]);
  check_scripted_stream(2, sizes, sent, 8, 2, 20, forms[2], true);
  check_scripted_stream(1, sizes, sent, 8, 2, 300, forms[2], true);
}

// ---- a. the planned roles of every rank, executed over fake pages ----

namespace {

// The launches of a recorded run: launch 2p is phase p's verification call,
// 2p + 1 its timed call, each with the ranks that made one.  A call's phase
// is the number of allgathers its rank has behind it.
std::vector<std::vector<std::pair<int, StreamCall>>> stream_launches(const std::vector<StreamRun>& runs) {
  std::vector<std::vector<std::pair<int, StreamCall>>> out;
  for (size_t r = 0; r < runs.size(); ++r) {
    size_t phase = 0, next = 0;
    for (char c : runs[r].log) {
      if (c == 'a') ++phase;
      if (c != 'v' && c != 't') continue;
      const size_t launch = 2 * phase + (c == 't' ? 1 : 0);
      if (out.size() <= launch) out.resize(launch + 1);
      out[launch].emplace_back(static_cast<int>(r), runs[r].calls[next++]);
    }
    EXPECT(next == runs[r].calls.size());
  }
  return out;
}

// A change to a planned role before it is executed (rank, launch, layout, role).
using StreamMutation = std::function<void(int, size_t, const StreamLayout&, StreamRolePlan*)>;

// A page is kept in 64-bit words; every offset the model uses is a byte
// offset that launch() has seen to be a multiple of 8.
uint64_t page_get64(const std::vector<uint64_t>& page, size_t at) { return page[at / 8]; }
void page_put64(std::vector<uint64_t>* page, size_t at, uint64_t v) { (*page)[at / 8] = v; }

// The kernel's protocol (stream.hip; StreamWave in
// tests/test_kernels_stream_gpu.py) on one array of layout.total bytes per rank.
struct StreamModel {
  struct Wave {
    int rank;
    StreamRolePlan p;
    int i = 0;
    bool done = false;
    uint64_t wrong = 0;
  };
  struct Write {
    int page;
    size_t begin, end;
    size_t wave;
  };

  int n;
  StreamLayout lay;
  std::vector<std::vector<uint64_t>> pages;
  std::vector<std::string> bad;  // "liveness: ...", "correctness:", "containment:", "exclusive:", "continuity:", "order:", "scratch:"

  explicit StreamModel(int nranks) : n(nranks) {}
  // As setup_once zeroes every page of a new geometry.
  void reset(const StreamLayout& l) {
    lay = l;
    pages.assign(static_cast<size_t>(n), std::vector<uint64_t>(l.total / 8, 0));
  }
  void note(const char* kind, size_t launch, const Wave& w, const std::string& what) {
    if (bad.size() < 50)
      bad.push_back(strfmt("%s launch %zu rank %d %s %d channel %d: %s", kind, launch, w.rank, w.p.sender ? "to" : "from",
                           w.p.peer, w.p.channel, what.c_str()));
  }

  // One message of a wave, if it can move.
  bool step(Wave* w) {
    const StreamRolePlan& p = w->p;
    std::vector<uint64_t>& own = pages[static_cast<size_t>(w->rank)];
    const uint64_t seq = p.base + static_cast<uint64_t>(w->i) + 1;
    const size_t nvec = p.bytes / 16;
    if (p.sender) {
      if (w->i == p.iters) {  // leaves only when the ring is consumed
        if (page_get64(own, p.in_flag) < p.base + static_cast<uint64_t>(p.iters)) return false;
        w->done = true;
        return true;
      }
      if (w->i >= p.depth && page_get64(own, p.in_flag) < seq - static_cast<uint64_t>(p.depth)) return false;
      std::vector<uint64_t>& ring = pages[static_cast<size_t>(p.ring_rank)];
      const size_t slot = p.ring + static_cast<size_t>(w->i % p.depth) * p.bytes;
      for (size_t j = 0; j < nvec; ++j) {
        page_put64(&ring, slot + 16 * j, seq);
        page_put64(&ring, slot + 16 * j + 8, j);
      }
      page_put64(&pages[static_cast<size_t>(p.out_rank)], p.out_flag, seq);
    } else {
      if (w->i == p.iters) {
        w->done = true;
        return true;
      }
      if (page_get64(own, p.in_flag) < seq) return false;
      const std::vector<uint64_t>& ring = pages[static_cast<size_t>(p.ring_rank)];
      const size_t slot = p.ring + static_cast<size_t>(w->i % p.depth) * p.bytes;
      for (size_t j = 0; j < nvec; ++j)  // every vector, whatever the role's check mode
        if (page_get64(ring, slot + 16 * j) != seq || page_get64(ring, slot + 16 * j + 8) != j) ++w->wrong;
      page_put64(&pages[static_cast<size_t>(p.out_rank)], p.out_flag, seq);
    }
    ++w->i;
    return true;
  }

  // One launch: the planned roles of every rank that called.
  void launch(size_t index, std::vector<Wave> waves) {
    std::vector<Write> writes;
    bool runnable = true;
    for (size_t k = 0; k < waves.size(); ++k) {
      const Wave& w = waves[k];
      const StreamRolePlan& p = w.p;
      const int c = p.channel;
      const bool self = p.peer == w.rank;
      const size_t ring_end = p.ring + static_cast<size_t>(std::min(p.iters, p.depth)) * p.bytes;
      // Inside the pages at all, or nothing below may touch them.
      if (p.out_rank < 0 || p.out_rank >= n || p.ring_rank < 0 || p.ring_rank >= n || p.out_flag + 8 > lay.total ||
          p.in_flag + 8 > lay.total || ring_end > lay.total || p.depth < 1 || p.bytes < 16 || p.bytes % 16 || p.out_flag % 8 ||
          p.in_flag % 8 || p.ring % 16) {
        note("containment:", index, w, "outside every page, or misaligned");
        runnable = false;
        continue;
      }
      // Containment: the sender writes the ring and tail of its inbox slot in
      // the receiver's page, the receiver the head line of its own rank in
      // the sender's page; the self path has slot and line n.
      if (p.sender) {
        const int slot = self ? n : w.rank;
        if (p.ring_rank != p.peer || p.ring < lay.ring(slot, c) || ring_end > lay.ring(slot, c) + lay.ring_bytes)
          note("containment:", index, w, strfmt("ring at %zu of rank %d's page", p.ring, p.ring_rank));
        if (p.out_rank != p.peer || p.out_flag != lay.tail(slot, c))
          note("containment:", index, w, strfmt("tail at %zu of rank %d's page", p.out_flag, p.out_rank));
        if (p.in_flag != lay.head(self ? n : p.peer, c)) note("containment:", index, w, strfmt("waits for the head at %zu", p.in_flag));
        writes.push_back({p.ring_rank, p.ring, ring_end, k});
      } else {
        if (p.out_rank != p.peer || p.out_flag != lay.head(self ? n : w.rank, c))
          note("containment:", index, w, strfmt("head at %zu of rank %d's page", p.out_flag, p.out_rank));
        const int slot = self ? n : p.peer;
        if (p.ring_rank != w.rank || p.ring != lay.ring(slot, c) || p.in_flag != lay.tail(slot, c))
          note("containment:", index, w, strfmt("reads the ring at %zu, the tail at %zu", p.ring, p.in_flag));
      }
      writes.push_back({p.out_rank, p.out_flag, p.out_flag + 8, k});
      // Continuity: nothing is ever reset, so the role counts on from what
      // its two flag words hold.
      const uint64_t in = page_get64(pages[static_cast<size_t>(w.rank)], p.in_flag);
      const uint64_t outv = page_get64(pages[static_cast<size_t>(p.out_rank)], p.out_flag);
      if (in != p.base || outv != p.base)
        note("continuity:", index, w, strfmt("base %llu, its flags hold %llu and %llu", p.base, static_cast<unsigned long long>(in),
                                             static_cast<unsigned long long>(outv)));
    }
    // Exclusivity: no byte has two writers in one launch.
    std::sort(writes.begin(), writes.end(), [](const Write& a, const Write& b) {
      return a.page != b.page ? a.page < b.page : a.begin < b.begin;
    });
    for (size_t k = 1; k < writes.size(); ++k)
      if (writes[k].page == writes[k - 1].page && writes[k].begin < writes[k - 1].end)
        note("exclusive:", index, waves[writes[k].wave],
             strfmt("byte %zu of rank %d's page is also written by rank %d", writes[k].begin, writes[k].page,
                    waves[writes[k - 1].wave].rank));
    // One rank's roles: receivers first, then senders, channels ascending;
    // status blocks and stamp regions share no 256-byte block and fit the
    // scratch of that many roles.
    for (size_t k = 0; k < waves.size(); ++k) {
      size_t first = k, count = 0;
      while (first > 0 && waves[first - 1].rank == waves[k].rank) --first;
      while (first + count < waves.size() && waves[first + count].rank == waves[k].rank) ++count;
      const StreamRolePlan& p = waves[k].p;
      const size_t pos = k - first;
      if (pos > 0) {
        const StreamRolePlan& q = waves[k - 1].p;
        if ((p.sender == q.sender && p.channel != q.channel + 1) || (p.sender != q.sender && (q.sender || p.channel != 0)))
          note("order:", index, waves[k], "receivers first, then senders, channels ascending");
        const size_t q_end = q.stamps + 8 * (static_cast<size_t>(q.iters) + 2);
        if (p.status != q.status + 256 || p.stamps % 256 || (q_end + 255) / 256 * 256 > p.stamps)
          note("scratch:", index, waves[k], "a status block or stamp region shares a 256-byte block with its neighbour's");
      } else if (p.status != 0 || p.stamps != 256 * 16) {
        note("scratch:", index, waves[k], "the first role's status block and stamps");
      }
      if (p.stamps + 8 * (static_cast<size_t>(p.iters) + 2) > StreamScratch::used(count, p.iters) || count > 16)
        note("scratch:", index, waves[k], "beyond what the launch copies back");
    }
    if (!runnable) return;
    // Round-robin, one message of each role a turn, until none can move.
    for (bool moved = true; moved;) {
      moved = false;
      for (Wave& w : waves)
        if (!w.done && step(&w)) moved = true;
    }
    for (const Wave& w : waves) {
      if (!w.done) note("liveness:", index, w, strfmt("waits at message %d of %d", w.i, w.p.iters));
      if (w.wrong) note("correctness:", index, w, strfmt("%llu wrong vectors", static_cast<unsigned long long>(w.wrong)));
    }
  }
};

// A recorded run planned and executed under each geometry in turn, with the
// same planners throughout: what a second stream_setup() does in between is
// reset() on every rank and zeroed pages.
std::vector<std::string> stream_model_violations(const std::vector<StreamRun>& runs, const std::vector<StreamLayout>& geometries,
                                                 const StreamMutation& mutate = nullptr) {
  const int n = static_cast<int>(runs.size());
  const auto launches = stream_launches(runs);
  StreamModel model(n);
  std::vector<StreamPlanner> planners;
  for (int r = 0; r < n; ++r) planners.emplace_back(r, n);
  for (const StreamLayout& lay : geometries) {
    model.reset(lay);
    for (StreamPlanner& p : planners) p.reset(lay);
    for (size_t l = 0; l < launches.size(); ++l) {
      std::vector<StreamModel::Wave> waves;
      for (const auto& rc : launches[l]) {
        const StreamCall& c = rc.second;
        for (StreamRolePlan role : planners[static_cast<size_t>(rc.first)].plan(c.send_to, c.recv_from, c.bytes, c.iters, c.check_all)) {
          if (mutate) mutate(rc.first, l, lay, &role);
          StreamModel::Wave w;
          w.rank = rc.first;
          w.p = role;
          waves.push_back(w);
        }
      }
      model.launch(l, std::move(waves));
    }
  }
  return model.bad;
}

bool has_violation(const std::vector<std::string>& bad, const char* kind) {
  for (const auto& s : bad)
    if (s.rfind(kind, 0) == 0) return true;
  return false;
}

void expect_no_stream_violations(const std::vector<std::string>& bad, const std::string& what) {
  EXPECT(bad.empty());
  for (size_t i = 0; i < bad.size() && i < 5; ++i) std::fprintf(stderr, "    %s: %s\n", what.c_str(), bad[i].c_str());
}

const std::vector<Direction> kBothForms{Direction::Uni, Direction::Bi};

}  // namespace

TEST(test_stream_plan_against_ring_model) {
  // 16, 112 and 4096 bytes in one run: the layout's slots are larger than
  // most of the messages sent into them.
  const std::vector<size_t> sizes{16, 100, 4096};
  for (int n : {1, 2, 3, 4, 5, 8})
    for (int depth : {1, 8})
      for (int iters : {1, 3, 3 * depth + 1}) {
        if (depth == 1 && iters == 3) continue;  // 3 * depth + 1 = 4 covers it
        // Channels and depth only pass through run_device_stream: one
        // recording serves both channel counts.
        const auto runs = scripted_stream(n, sizes, depth, 1, iters, kBothForms);
        for (int channels : {1, 8}) {
          // Then laid out again, as a second stream_setup with other arguments does.
          const std::vector<StreamLayout> geometries{stream_layout(n, channels, depth, 4096),
                                                     stream_layout(n, channels == 1 ? 2 : 3, depth + 2, 4112)};
          expect_no_stream_violations(stream_model_violations(runs, geometries),
                                      strfmt("n %d depth %d iters %d channels %d", n, depth, iters, channels));
        }
      }
}

// The model has teeth: each of these one-line changes to the planned roles
// breaks the contract, and the model must say so.
TEST(test_stream_model_rejects_mutations) {
  const std::vector<size_t> sizes{16, 100};
  // 300 messages: the verification launch sends 256 of them, the timed one 300.
  const int depth = 8, channels = 2, iters = 300;
  const auto self = scripted_stream(1, sizes, depth, channels, iters, kBothForms);
  const auto three = scripted_stream(3, sizes, depth, channels, iters, kBothForms);
  const std::vector<StreamLayout> lay1{stream_layout(1, channels, depth, 112)}, lay3{stream_layout(3, channels, depth, 112)};
  EXPECT(stream_model_violations(self, lay1).empty() && stream_model_violations(three, lay3).empty());
  {  // the self path in slot `rank` instead of slot n
    const auto bad = stream_model_violations(self, lay1, [](int rank, size_t, const StreamLayout& l, StreamRolePlan* r) {
      (r->sender ? r->out_flag : r->in_flag) = l.tail(rank, r->channel);
      r->ring = l.ring(rank, r->channel);
    });
    EXPECT(has_violation(bad, "containment:"));
  }
  {  // the receiver's credit on line recv_from instead of its own rank
    const auto bad = stream_model_violations(three, lay3, [](int, size_t, const StreamLayout& l, StreamRolePlan* r) {
      if (!r->sender) r->out_flag = l.head(r->peer, r->channel);
    });
    EXPECT(has_violation(bad, "containment:") && has_violation(bad, "liveness:"));
  }
  {  // the sender's ring in slot send_to instead of its own rank
    const auto bad = stream_model_violations(three, lay3, [](int, size_t, const StreamLayout& l, StreamRolePlan* r) {
      if (r->sender) r->ring = l.ring(r->peer, r->channel), r->out_flag = l.tail(r->peer, r->channel);
    });
    EXPECT(has_violation(bad, "containment:") && has_violation(bad, "liveness:"));
  }
  {  // a base not advanced after a launch: the timed launch starts where the verification did
    const auto bad = stream_model_violations(three, lay3, [](int, size_t launch, const StreamLayout&, StreamRolePlan* r) {
      if (launch % 2 == 1) r->base -= 256;
    });
    EXPECT(has_violation(bad, "continuity:"));
  }
  {  // a base advanced by verify_iters where the launch sent iters
    const auto bad = stream_model_violations(three, lay3, [](int, size_t, const StreamLayout&, StreamRolePlan* r) {
      r->base -= r->base / (256 + 300) * (300 - 256);
    });
    EXPECT(has_violation(bad, "continuity:"));
  }
  {  // the two channels of a flow share a head line
    const auto bad = stream_model_violations(three, lay3, [](int, size_t, const StreamLayout&, StreamRolePlan* r) {
      if (r->channel == 1) (r->sender ? r->in_flag : r->out_flag) -= StreamLayout::kCreditLine;
    });
    EXPECT(has_violation(bad, "exclusive:"));
  }
}

TEST(test_stream_planner_refuses_bad_calls) {
  StreamPlanner p(1, 3);
  EXPECT(has_text(fatal_text([&] { p.plan(0, -1, 16, 1, false); }), "stream_setup() first"));
  p.reset(stream_layout(3, 2, 4, 100));
  EXPECT(has_text(fatal_text([&] { p.plan(3, -1, 16, 1, false); }), "bad peer"));
  EXPECT(has_text(fatal_text([&] { p.plan(-1, -2, 16, 1, false); }), "bad peer"));
  EXPECT(has_text(fatal_text([&] { p.plan(-1, -1, 16, 1, false); }), "nothing to send or receive"));
  EXPECT(has_text(fatal_text([&] { p.plan(1, -1, 16, 1, false); }), "the self path sends to and receives from the own rank"));
  EXPECT(has_text(fatal_text([&] { p.plan(1, 0, 16, 1, false); }), "the self path"));
  EXPECT(has_text(fatal_text([&] { p.plan(0, -1, 16, 0, false); }), "1..100000 messages"));
  EXPECT(has_text(fatal_text([&] { p.plan(0, -1, 16, 100001, false); }), "1..100000 messages"));
  EXPECT(has_text(fatal_text([&] { p.plan(0, -1, 113, 1, false); }), "messages of at most 112 bytes were set up"));
  // A refused call counts nothing; an accepted one counts its messages on
  // the lines it used only, and rounds its size up.
  for (auto v : p.sent()) EXPECT(v == 0);
  const auto roles = p.plan(0, 2, 100, 5, true);
  EXPECT(roles.size() == 4 && roles[0].bytes == 112 && !roles[0].sender && roles[3].sender && roles[3].channel == 1);
  EXPECT(p.sent() == (std::vector<unsigned long long>{5, 5, 0, 0, 0, 0, 0, 0}));
  EXPECT(p.recvd() == (std::vector<unsigned long long>{0, 0, 0, 0, 5, 5, 0, 0}));
  EXPECT(p.plan(1, 1, 16, 7, false)[0].base == 0 && p.plan(1, 1, 16, 1, false)[3].base == 7);
  EXPECT(p.sent()[6] == 8 && p.recvd()[7] == 8);
  p.reset(stream_layout(3, 1, 4, 100));
  EXPECT(p.sent() == (std::vector<unsigned long long>{0, 0, 0, 0}) && p.plan(0, 2, 16, 5, true)[0].base == 0);
}

// ---- c. the fold over scripted stamps ----

namespace {

constexpr double kStreamHz = 100e6;

// Role k's stamp i: exact integers, irregular steps, every role with its own
// start.  Channel 0 (k % channels == 0) starts neither first nor last and
// ends neither first nor last where there are four channels.
uint64_t scripted_stamp(size_t k, size_t channels, size_t i) {
  static const uint64_t start[4] = {500, 100, 900, 300};
  uint64_t t = 1000000 + start[k % channels % 4] + 13 * (k / channels);
  for (size_t j = 0; j < i; ++j) t += 3 + (7 * j + 5 * (k % channels) + (k / channels)) % 11;
  return t;
}

constexpr unsigned char kGuard = 0xAB;

// The scratch image a launch of `plan` leaves: exactly as many bytes as the
// transport copies back (the ASan build sees any read beyond), guard bytes
// wherever the kernel writes nothing (the padding of the status blocks, the
// stamps a role does not write), status words clean.
std::vector<unsigned char> scripted_scratch(const std::vector<StreamRolePlan>& plan, size_t channels, int iters) {
  const size_t stride = (static_cast<size_t>(iters) + 2 + 31) / 32 * 32;  // entries: whole 256-byte blocks
  std::vector<unsigned char> img(16 * 256 + plan.size() * stride * 8, kGuard);
  for (size_t k = 0; k < plan.size(); ++k) {
    EXPECT(plan[k].status == 256 * k && plan[k].stamps == 16 * 256 + k * stride * 8);
    std::memset(img.data() + 256 * k, 0, 8);
    const size_t written = plan[k].sender ? static_cast<size_t>(iters) + 2 : static_cast<size_t>(iters);
    for (size_t i = 0; i < written; ++i) {
      const uint64_t v = scripted_stamp(k, channels, i);
      std::memcpy(img.data() + 16 * 256 + (k * stride + i) * 8, &v, 8);
    }
  }
  return img;
}

}  // namespace

TEST(test_stream_fold_scripted_stamps) {
  EXPECT(StreamScratch::used(3, 30) == 16 * 256 + 3 * 32 * 8 && StreamScratch::used(3, 31) == 16 * 256 + 3 * 64 * 8);
  const int n = 4, me = 0;
  for (size_t channels : {size_t{1}, size_t{4}})
    for (int iters : {1, 5, 31, 70})
      for (size_t bytes : {size_t{16}, size_t{4096}})
        for (bool check_all : {false, true})
          for (int form = 0; form < 3; ++form) {  // sender and receiver, sender only, receiver only
            const int send_to = form == 2 ? -1 : 1, recv_from = form == 1 ? -1 : 3;
            StreamPlanner planner(me, n);
            planner.reset(stream_layout(n, static_cast<int>(channels), 8, 4096));
            const auto plan = planner.plan(send_to, recv_from, bytes, iters, check_all);
            EXPECT(plan.size() == channels * (form == 0 ? 2 : 1));
            const auto img = scripted_scratch(plan, channels, iters);
            EXPECT(img.size() == StreamScratch::used(plan.size(), iters));
            const StreamFold f = fold_stream_stamps(plan, img.data(), img.size(), kStreamHz);
            EXPECT(f.ok() && f.role == -1 && !f.deadline && f.wrong == 0 && f.times.wrong_vectors == 0);
            const auto& t = f.times;
            EXPECT(t.sent == (send_to >= 0) && t.received == (recv_from >= 0));
            // Expected values by plain loops over the script.
            uint64_t s_min = ~0ull, s_max = 0, r_min = ~0ull, r_max = 0;
            size_t s_min_k = 0, s_max_k = 0, r_min_k = 0, r_max_k = 0, first_sender = plan.size();
            const size_t it = static_cast<size_t>(iters);
            for (size_t k = 0; k < plan.size(); ++k) {
              if (plan[k].sender) {
                if (first_sender == plan.size()) first_sender = k;
                if (scripted_stamp(k, channels, 0) < s_min) s_min = scripted_stamp(k, channels, 0), s_min_k = k;
                if (scripted_stamp(k, channels, it + 1) > s_max) s_max = scripted_stamp(k, channels, it + 1), s_max_k = k;
              } else {
                if (scripted_stamp(k, channels, 0) < r_min) r_min = scripted_stamp(k, channels, 0), r_min_k = k;
                if (scripted_stamp(k, channels, it - 1) > r_max) r_max = scripted_stamp(k, channels, it - 1), r_max_k = k;
              }
            }
            if (channels == 4) {  // channel 0 decides neither end of either span
              if (t.sent) EXPECT(plan[s_min_k].channel != 0 && plan[s_max_k].channel != 0);
              if (t.received) EXPECT(plan[r_min_k].channel != 0 && plan[r_max_k].channel != 0);
            }
            if (t.sent) {
              EXPECT(t.send_span_s == static_cast<double>(s_max - s_min) / kStreamHz && t.send_span_s > 0);
              EXPECT(plan[first_sender].channel == 0);
              EXPECT(t.gap_us.size() == it);
              for (size_t i = 0; i < it && i < t.gap_us.size(); ++i)
                EXPECT(t.gap_us[i] == static_cast<double>(scripted_stamp(first_sender, channels, i + 1) -
                                                          scripted_stamp(first_sender, channels, i)) / kStreamHz * 1e6);
            } else {
              EXPECT(t.send_span_s == 0 && t.gap_us.empty());
            }
            if (t.received) {
              EXPECT(t.recv_span_s == static_cast<double>(r_max - r_min) / kStreamHz);
              EXPECT(iters > 1 || channels > 1 || t.recv_span_s == 0);
              const uint64_t per_message = check_all ? bytes / 16 : (bytes == 16 ? 1 : 2);
              EXPECT(t.checked_vectors == channels * it * per_message);
            } else {
              EXPECT(t.recv_span_s == 0 && t.checked_vectors == 0);
            }

            // A deadline bit, or a wrong count, in exactly one role's status
            // block: that role is reported, with its direction and its peer.
            for (size_t k = 0; k < plan.size(); ++k) {
              auto late = img;
              const unsigned int bit = 1;
              std::memcpy(late.data() + 256 * k, &bit, 4);
              const StreamFold d = fold_stream_stamps(plan, late.data(), late.size(), kStreamHz);
              EXPECT(!d.ok() && d.role == static_cast<int>(k) && d.deadline && d.wrong == 0);
              auto wrong = img;
              const unsigned int count = 7 + static_cast<unsigned int>(k);
              std::memcpy(wrong.data() + 256 * k + 4, &count, 4);
              const StreamFold w = fold_stream_stamps(plan, wrong.data(), wrong.size(), kStreamHz);
              EXPECT(!w.ok() && w.role == static_cast<int>(k) && !w.deadline && w.wrong == count &&
                     w.times.wrong_vectors == count);
              if (w.role == static_cast<int>(k)) {
                const StreamRolePlan& r = plan[k];
                const bool sender = k >= (form == 0 ? channels : 0) && form != 2;
                EXPECT(r.sender == sender && r.peer == (sender ? 1 : 3) && r.channel == static_cast<int>(k % channels));
              }
              if (k + 1 < plan.size()) {  // two roles fail: the first in launch order is named
                std::memcpy(wrong.data() + 256 * (k + 1), &bit, 4);
                EXPECT(fold_stream_stamps(plan, wrong.data(), wrong.size(), kStreamHz).role == static_cast<int>(k));
              }
            }
          }
  // The fold reads no further than the image it is given.
  StreamPlanner planner(0, 2);
  planner.reset(stream_layout(2, 1, 8, 4096));
  const auto plan = planner.plan(1, 1, 64, 40, false);
  const auto img = scripted_scratch(plan, 1, 40);
  EXPECT(has_text(fatal_text([&] { fold_stream_stamps(plan, img.data(), img.size() - 64 * 8 + 41 * 8, kStreamHz); }),
                  "outside the scratch"));
  EXPECT(fold_stream_stamps(plan, img.data(), img.size() - 64 * 8 + 42 * 8, kStreamHz).ok());
}


int main(int argc, char** argv) {
  const char* only = argc > 1 ? argv[1] : nullptr;
  int ran = 0;
  for (auto& tc : registry()) {
    if (only && !std::strstr(tc.name, only)) continue;
    int before = g_failures;
    std::printf("[ RUN  ] %s\n", tc.name);
    std::fflush(stdout);
    tc.fn();
    std::printf("[ %s ] %s\n", g_failures == before ? " OK " : "FAIL", tc.name);
    ++ran;
  }
  std::printf("%d tests, %d checks, %d failures\n", ran, g_checks.load(), g_failures.load());
  return g_failures ? 1 : 0;
}
