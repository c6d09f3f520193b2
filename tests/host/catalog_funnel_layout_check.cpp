// Host-only check of the two workspaces of include/unirec_hip_funnel.h (unirec_amd/csrc/catalog_layout.hip.h: funnel_select_layout,
// funnel_rerank_layout), built with -fsanitize=address,undefined by tests/test_catalog_funnel_host.py.  Over a grid of B, N, dim, K and
// segments: each region starts on a 16-byte boundary, no two regions overlap, the last one ends inside `need`, and `need` is the closed
// form of the documented layout (written out here a second time, not taken from the carver) -- in which neither row stride appears.
// Exit status 0 and "ok <cases>" on success.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "catalog_layout.hip.h"

namespace {

struct region {
  const char* name;
  int64_t at, bytes;
};

int64_t pad16(int64_t n) { return (n + 15) / 16 * 16; }
int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

[[noreturn]] void fail(const char* what, const char* entry, const char* name, long long a, long long b) {
  std::fprintf(stderr, "catalog_funnel_layout_check: %s: %s %s (%lld, %lld)\n", entry, what, name, a, b);
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

int main() {
  long cases = 0;
  for (int32_t B : {0, 1, 3, 17, 64, 512, 2000})
    for (int64_t N : {(int64_t)0, (int64_t)1, (int64_t)1500, (int64_t)5003, (int64_t)1 << 20, (int64_t)1 << 30})
      for (int64_t chunk_rows : {(int64_t)0, (int64_t)1024, (int64_t)1 << 18})
        for (int32_t K : {1, 128, 129, 1000, 1024})
          for (int32_t dim : {8, 40, 256, 1032, 2048})
            for (int32_t segments : {0, 1, 3, 16}) {
              // rows: the caller's figure or a chunk buffer near 64 MB, at most N rounded up to 1024, at least one tile
              const int64_t n_up = cdiv(N, 1024) * 1024;
              int64_t rows = chunk_rows > 0 ? chunk_rows : ((int64_t)64 << 20) / (4 * (int64_t)std::max(B, 1)) / 1024 * 1024;
              rows = std::max<int64_t>(std::min(rows, n_up), 1024);
              const int gw = segments > 0 ? segments : (int)std::min<int64_t>(std::max<int64_t>(1024 / std::max(B, 1), 1), 8);
              const int64_t ubf = (int64_t)B * dim * 2, vec = (int64_t)B * 4, chunk = (int64_t)B * rows * 4;
              const int64_t list = (int64_t)B * gw * K * 4, count = (int64_t)B * gw * 4;
              const coarse_deep_plan p = funnel_select_layout(B, N, dim, K, chunk_rows, segments);
              if (p.rows != rows) fail("chunk rows", "funnel_select", "rows", p.rows, rows);
              if (p.gw != gw) fail("segments", "funnel_select", "gw", p.gw, gw);
              check("funnel_select", p.need, std::max<int64_t>(16, pad16(ubf) + 2 * pad16(vec) + pad16(chunk) + 2 * pad16(list) + pad16(count)),
                    {{"user", p.user, ubf}, {"inv_u", p.inv_u, vec}, {"ref", p.ref, vec}, {"chunk", p.chunk, chunk},
                     {"list_score", p.list_score, list}, {"list_index", p.list_index, list}, {"count", p.count, count}});

              const int64_t scores = (int64_t)B * K * 4;      // K stands for K_in here
              const deep_rerank_plan r = funnel_rerank_layout(B, K);
              check("funnel_rerank", r.need, std::max<int64_t>(16, pad16(vec) + pad16(scores)), {{"inv_u", r.inv_u, vec}, {"score", r.score, scores}});
              ++cases;
            }
  std::printf("ok %ld\n", cases);
  return 0;
}
