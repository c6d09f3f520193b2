// Host-only check of the two workspaces of include/unirec_fp8.h (unirec_amd/csrc/catalog_layout.hip.h: fp8_select_layout,
// fp8_rerank_layout) and of the number format (unirec_amd/csrc/catalog_fp8_codec.hip.h), built with -fsanitize=address,undefined by
// tests/test_catalog_fp8_host.py.  Over a grid of B, N, D, K and segments: each region starts on a 16-byte boundary, no two regions
// overlap, the last one ends inside `need`, and `need` is the closed form of the documented layout (written out here a second time, not
// taken from the carver).  The codec: every non-NaN code decodes and encodes back to itself, every midpoint between neighbours goes to
// the even code, and the row exponent is the largest e with a 2^e <= 448 at the boundary mantissas.
// Exit status 0 and "ok <cases>" on success.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "catalog_layout.hip.h"
#include "catalog_fp8_codec.hip.h"

namespace {

struct region {
  const char* name;
  int64_t at, bytes;
};

int64_t pad16(int64_t n) { return (n + 15) / 16 * 16; }
int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

[[noreturn]] void fail(const char* what, const char* entry, const char* name, long long a, long long b) {
  std::fprintf(stderr, "catalog_fp8_layout_check: %s: %s %s (%lld, %lld)\n", entry, what, name, a, b);
  std::exit(1);
}

void check(const char* entry, int64_t need, int64_t want, std::vector<region> r) {
  if (need != want) fail("need differs from the closed form", entry, "", need, want);
  std::sort(r.begin(), r.end(), [](const region& x, const region& y) { return x.at < y.at || (x.at == y.at && x.bytes < y.bytes); });
  for (size_t i = 0; i < r.size(); ++i) {
    if (r[i].at < 0 || (r[i].at % 16) != 0) fail("misaligned region", entry, r[i].name, r[i].at, r[i].bytes);
    const int64_t end = r[i].at + r[i].bytes;
    if (i + 1 < r.size() && end > r[i + 1].at) fail("region overlaps the next one", entry, r[i].name, end, r[i + 1].at);
    if (end > need) fail("region ends past need", entry, r[i].name, end, need);
  }
}

}  // namespace

// the codec against the format, written out here a second time: value = m 2^-9 (e == 0) or (8 + m) 2^(e - 10)
double code_value(int c) {
  const int e = (c >> 3) & 15, m = c & 7;
  double v = e == 0 ? m / 512.0 : (8 + m) / 1024.0;
  for (int i = 0; e > 0 && i < e; ++i) v *= 2.0;
  return (c & 0x80) ? -v : v;
}

void check_codec() {
  for (int c = 0; c < 256; ++c) {
    if ((c & 0x7f) == 0x7f) continue;                           // the NaN codes
    const float v = fp8_decode((uint32_t)c);
    if ((double)v != code_value(c) || (c == 0x80 && !std::signbit(v))) fail("decode", "codec", "value", c, 0);
    if (fp8_encode(v) != (uint32_t)c) fail("encode(decode(c)) != c", "codec", "code", c, fp8_encode(v));
    if ((c & 0x7f) < 0x7e) {                                    // the midpoint to the next code of the same sign goes to the even one
      const float mid = (float)((code_value(c) + code_value(c + 1)) / 2);
      const uint32_t even = (c & 1) ? (uint32_t)c + 1 : (uint32_t)c;
      if (fp8_encode(mid) != even) fail("a tie must go to the even code", "codec", "midpoint", c, fp8_encode(mid));
      if (fp8_encode(std::nextafterf(mid, 1e9f * (c & 0x80 ? -1.f : 1.f))) != (uint32_t)c + 1) fail("above a tie", "codec", "midpoint", c, 1);
      if (fp8_encode(std::nextafterf(mid, 0.f)) != (uint32_t)c) fail("below a tie", "codec", "midpoint", c, -1);
    }
  }
  // the row exponent: the largest e in [-64, 64] with a 2^e <= 448, at the boundary mantissa 0.875, at 0.5 and at their neighbours
  for (int x = -80; x <= 80; ++x)
    for (float m : {0.5f, std::nextafterf(0.5f, 1.f), std::nextafterf(0.875f, 0.f), 0.875f, std::nextafterf(0.875f, 1.f), std::nextafterf(1.f, 0.f)}) {
      const float a = std::ldexp(m, x);
      int best = -64;
      for (int e = -64; e <= 64; ++e)
        if (std::ldexp((double)a, e) <= 448.0) best = e;
      if (fp8_row_exponent(fp8_f32_bits(a)) != best) fail("row exponent", "codec", "e", fp8_row_exponent(fp8_f32_bits(a)), best);
      if (fp8_pow2(best) != std::ldexp(1.0f, best)) fail("2^e", "codec", "pow2", best, 0);
    }
  if (fp8_row_exponent(0) != 0 || fp8_row_exponent(0x7f800000u) != 0 || fp8_row_exponent(0x7fc00000u) != 0 || fp8_row_exponent(1) != 64)
    fail("row exponent", "codec", "special", 0, 0);
}

int main() {
  check_codec();
  long cases = 0;
  for (int32_t B : {0, 1, 3, 17, 64, 512, 2000})
    for (int64_t N : {(int64_t)0, (int64_t)1, (int64_t)1500, (int64_t)5003, (int64_t)1 << 20, (int64_t)1 << 30})
      for (int64_t chunk_rows : {(int64_t)0, (int64_t)1024, (int64_t)1 << 18})
        for (int32_t K : {1, 128, 129, 1000, 1024})
          for (int32_t D : {16, 48, 256, 1056, 2048})
            for (int32_t segments : {0, 1, 3, 16}) {
              // rows: the caller's figure or a chunk buffer near 64 MB, at most N rounded up to 1024, at least one tile
              const int64_t n_up = cdiv(N, 1024) * 1024;
              int64_t rows = chunk_rows > 0 ? chunk_rows : ((int64_t)64 << 20) / (4 * (int64_t)std::max(B, 1)) / 1024 * 1024;
              rows = std::max<int64_t>(std::min(rows, n_up), 1024);
              const int gw = segments > 0 ? segments : (int)std::min<int64_t>(std::max<int64_t>(1024 / std::max(B, 1), 1), 8);
              const int64_t ubf = (int64_t)B * D, vec = (int64_t)B * 4, chunk = (int64_t)B * rows * 4;
              const int64_t list = (int64_t)B * gw * K * 4, count = (int64_t)B * gw * 4;
              const fp8_select_plan p = fp8_select_layout(B, N, D, K, chunk_rows, segments);
              if (p.rows != rows) fail("chunk rows", "fp8_select", "rows", p.rows, rows);
              if (p.gw != gw) fail("segments", "fp8_select", "gw", p.gw, gw);
              check("fp8_select", p.need, std::max<int64_t>(16, pad16(ubf) + 3 * pad16(vec) + pad16(chunk) + 2 * pad16(list) + pad16(count)),
                    {{"user", p.user, ubf}, {"inv_u", p.inv_u, vec}, {"scale_u", p.scale_u, vec}, {"ref", p.ref, vec}, {"chunk", p.chunk, chunk},
                     {"list_score", p.list_score, list}, {"list_index", p.list_index, list}, {"count", p.count, count}});

              const int64_t scores = (int64_t)B * K * 4;      // K stands for K_in here
              const deep_rerank_plan r = fp8_rerank_layout(B, K);
              check("fp8_rerank", r.need, std::max<int64_t>(16, pad16(vec) + pad16(scores)), {{"inv_u", r.inv_u, vec}, {"score", r.score, scores}});
              ++cases;
            }
  std::printf("ok %ld\n", cases);
  return 0;
}
