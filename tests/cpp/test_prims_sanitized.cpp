// TEST INFRASTRUCTURE (host only): drives the scan / select / unique / sort primitives of prims.hip through the C ABI against the AddressSanitizer +
// alignment-checking build of the host SIMT interpreter library (HIPSIM_ASAN=1 python tests/hipsim/build.py).  This program is linked with
// -fsanitize=address itself, so the sanitizer runtime is its own.  On the interpreter "device" memory is host memory: every array handed to the library
// is a heap block of EXACTLY the bytes the call may touch, so that a load or store one item out of range lands in a redzone and aborts the program,
// and so does a 16-byte access to an address that is not 16-byte aligned.  (The outputs of select / unique have their capacity of n items, filled
// with a guard word that must survive from out[count] on.)  A wrong answer exits 1.
// Built and run by tests/test_sim_cpu.py::test_prims_under_address_and_alignment_sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "ghicp_c.h"

namespace {

constexpr uint32_t GUARD = 0xA5A5A5A5u;
ghicp_ctx* ctx = nullptr;
int failures = 0;
uint64_t rng_state = 0x9E3779B97F4A7C15ull;

uint32_t rnd() {  // splitmix64, upper half
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

void fail(const char* what, long long n, int a, long long at) {
  if (failures++ < 20) fprintf(stderr, "FAIL %s n=%lld case=%d at %lld (%s)\n", what, n, a, at, ghicp_last_error(ctx));
}

// a heap block of exactly `bytes` bytes (at least one) that starts on a 256-byte boundary
struct Block {
  void* p = nullptr;
  explicit Block(size_t bytes) {
    if (posix_memalign(&p, 256, bytes ? bytes : 1) != 0) abort();
  }
  ~Block() { free(p); }
  Block(const Block&) = delete;
  template <typename T> T* as() const { return static_cast<T*>(p); }
};

const long long SIZES[] = {1, 15, 16, 17, 63, 64, 65, 255, 256, 4095, 4096, 4097, 8192, 65537, 1048576, 1048577};

void scan_cases() {
  for (long long n : SIZES)
    for (int off = 0; off < 4; off++) {  // the range starts `off` words past a 256-byte boundary and ends with the block
      Block b((size_t)(off + n) * 4);
      uint32_t* base = b.as<uint32_t>();
      for (int k = 0; k < off; k++) base[k] = 0xA5A5A5A5u;
      std::vector<uint32_t> want((size_t)n);
      uint64_t run = 0;
      for (long long i = 0; i < n; i++) {
        const uint32_t v = rnd();
        base[off + i] = v;
        run += v;
        want[(size_t)i] = (uint32_t)(run & 0xFFFFFFFFull);
      }
      if (ghicp_scan_inclusive_u32(ctx, base + off, n) != GHICP_OK) { fail("scan rc", n, off, -1); continue; }
      for (long long i = 0; i < n; i++)
        if (base[off + i] != want[(size_t)i]) { fail("scan", n, off, i); break; }
      for (int k = 0; k < off; k++)
        if (base[k] != 0xA5A5A5A5u) fail("scan: word before the range", n, off, k);
    }
}

// flag patterns: 0 tile edges, 1 wave edges, 2 random half, 3 none, 4 all, 5 last item only, 6 random bytes of {0, 2, 0x80, 0xFF}
uint8_t flag_of(int pat, long long i, long long n) {
  switch (pat) {
    case 0: return (i % 4096 == 0 || i % 4096 == 4095) ? 1 : 0;
    case 1: return (i % 64 == 0 || i % 64 == 63) ? 1 : 0;
    case 2: return rnd() & 1u;
    case 3: return 0;
    case 4: return 1;
    case 5: return i == n - 1 ? 0xFF : 0;
    default: { static const uint8_t tab[4] = {0, 0x02, 0x80, 0xFF}; return tab[rnd() & 3u]; }
  }
}

void select_cases() {
  for (long long n : SIZES)
    for (int pat = 0; pat < 7; pat++)
      for (int with_vals = 0; with_vals < 2; with_vals++) {
        Block fb((size_t)n), vb((size_t)n * 4);
        uint8_t* f = fb.as<uint8_t>();
        uint32_t* v = vb.as<uint32_t>();
        std::vector<uint32_t> want;
        for (long long i = 0; i < n; i++) {
          f[i] = flag_of(pat, i, n);
          v[i] = rnd();
          if (f[i]) want.push_back(with_vals ? v[i] : (uint32_t)i);
        }
        Block ob((size_t)n * 4);
        std::fill(ob.as<uint32_t>(), ob.as<uint32_t>() + n, GUARD);
        int64_t count = -1;
        if (ghicp_select_flagged(ctx, f, with_vals ? v : nullptr, n, ob.as<uint32_t>(), &count) != GHICP_OK) { fail("select rc", n, pat, -1); continue; }
        if (count != (int64_t)want.size()) { fail("select count", n, pat, count); continue; }
        if (count && memcmp(ob.p, want.data(), want.size() * 4) != 0) fail("select", n, pat, with_vals);
        for (long long i = count; i < n; i++)
          if (ob.as<uint32_t>()[i] != GUARD) { fail("select: store past out[count]", n, pat, i); break; }
      }
}

void unique_cases() {
  const long long runs[] = {1, 64, 4096, 4097, 0 /* random */, -1 /* one run */};
  for (long long n : SIZES)
    for (int r = 0; r < 6; r++) {
      Block kb((size_t)n * 4);  // key[-1] and key[n] are out of range
      uint32_t* k = kb.as<uint32_t>();
      std::vector<uint32_t> want;
      uint32_t cur = 0;
      for (long long i = 0; i < n; i++) {
        const bool head = i == 0 || (runs[r] > 0 ? i % runs[r] == 0 : (runs[r] == 0 && (rnd() & 7u) == 0));
        if (head && i) cur += 1 + (rnd() & 3u);
        if (i == n - 1 && head) cur = 0xFFFFFFFFu;
        k[i] = cur;
        if (head) want.push_back(cur);
      }
      Block ob((size_t)n * 4);
      std::fill(ob.as<uint32_t>(), ob.as<uint32_t>() + n, GUARD);
      int64_t count = -1;
      if (ghicp_unique_sorted_u32(ctx, k, n, ob.as<uint32_t>(), &count) != GHICP_OK) { fail("unique rc", n, r, -1); continue; }
      if (count != (int64_t)want.size()) { fail("unique count", n, r, count); continue; }
      if (memcmp(ob.p, want.data(), want.size() * 4) != 0) fail("unique", n, r, 0);
      for (long long i = count; i < n; i++)
        if (ob.as<uint32_t>()[i] != GUARD) { fail("unique: store past out[count]", n, r, i); break; }
    }
}

template <typename K>
void sort_case(long long n, int bit_begin, int bit_end, bool with_vals) {
  Block kib((size_t)n * sizeof(K)), kob((size_t)n * sizeof(K)), vib((size_t)n * 4), vob((size_t)n * 4);
  K* ki = kib.as<K>();
  uint32_t* vi = vib.as<uint32_t>();
  for (long long i = 0; i < n; i++) {
    ki[i] = (K)(((uint64_t)rnd() << 32) | rnd());
    vi[i] = (uint32_t)(n - 1 - i);
  }
  const uint64_t mask = bit_end - bit_begin == 64 ? ~0ull : ((1ull << (bit_end - bit_begin)) - 1ull);
  std::vector<uint32_t> order((size_t)n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return (((uint64_t)ki[a] >> bit_begin) & mask) < (((uint64_t)ki[b] >> bit_begin) & mask); });
  if (ghicp_sort_pairs(ctx, (int)sizeof(K), ki, kob.p, with_vals ? vi : nullptr, with_vals ? vob.as<uint32_t>() : nullptr, n, bit_begin, bit_end) != GHICP_OK) {
    fail("sort rc", n, (int)sizeof(K), -1);
    return;
  }
  for (long long i = 0; i < n; i++)
    if (kob.as<K>()[i] != ki[order[(size_t)i]] || (with_vals && vob.as<uint32_t>()[i] != vi[order[(size_t)i]])) { fail("sort", n, (int)sizeof(K), i); break; }
}

void sort_cases() {
  for (long long n : {1ll, 63ll, 4096ll, 4097ll, 70001ll, 262144ll, 262145ll})
    for (int with_vals = 0; with_vals < 2; with_vals++) {
      sort_case<uint32_t>(n, 0, 16, with_vals != 0);
      sort_case<uint64_t>(n, 27, 43, with_vals != 0);
    }
  // aliased buffers are an argument error and nothing is written
  std::vector<uint32_t> a(3000), before;
  for (auto& x : a) x = rnd();
  before = a;
  if (ghicp_sort_pairs(ctx, 4, a.data(), a.data() + 500, nullptr, nullptr, 1000, 0, 8) != GHICP_ERR_ARG) fail("sort: overlapping keys accepted", 1000, 0, 0);
  if (ghicp_sort_pairs(ctx, 4, a.data(), a.data() + 1000, a.data() + 2000, a.data() + 2000, 1000, 0, 8) != GHICP_ERR_ARG) fail("sort: vals_in == vals_out accepted", 1000, 1, 0);
  if (a != before) fail("sort: a rejected call wrote", 1000, 2, 0);
}

}  // namespace

int main() {
  if (ghicp_ctx_create(0, &ctx) != GHICP_OK) { fprintf(stderr, "no context\n"); return 2; }
  scan_cases();
  select_cases();
  unique_cases();
  sort_cases();
  ghicp_ctx_destroy(ctx);
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("prims sanitized: ok\n");
  return 0;
}
