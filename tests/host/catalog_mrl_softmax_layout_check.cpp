// Host-only check of the workspace of include/unirec_hip_mrl_loss.h (unirec_amd/csrc/catalog_layout.hip.h: catalog_mrl_softmax_layout),
// built with -fsanitize=address,undefined by tests/test_catalog_mrl_softmax_host.py.  Over a grid of B, N, dims, chunk_rows and forward /
// forward + backward: each region starts on a 16-byte boundary, no two regions overlap, the last one ends inside `need`, `need` is the
// closed form of the documented layout (written out here a second time, not taken from the carver), the chunk rows follow the header's
// rule, and every plane's segment size and row splits are those ur_catalog_softmax's own plan takes on the slice at the same explicit
// chunk_rows -- what the bit contract rests on.  Exit status 0 and "ok <cases>" on success.
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

[[noreturn]] void fail(const char* what, const char* name, long long a, long long b) {
  std::fprintf(stderr, "catalog_mrl_softmax_layout_check: %s %s (%lld, %lld)\n", what, name, a, b);
  std::exit(1);
}

void check(int64_t need, int64_t want, std::vector<region> r) {
  if (need != want) fail("need differs from the closed form", "", need, want);
  std::sort(r.begin(), r.end(), [](const region& x, const region& y) { return x.at < y.at || (x.at == y.at && x.bytes < y.bytes); });
  for (size_t i = 0; i < r.size(); ++i) {
    if (r[i].at < 0 || (r[i].at % 16) != 0) fail("misaligned region", r[i].name, r[i].at, r[i].bytes);
    const int64_t end = r[i].at + r[i].bytes;
    if (i + 1 < r.size() && end > r[i + 1].at) fail("region overlaps the next one", r[i].name, end, r[i + 1].at);
    if (end > need) fail("region ends past need", r[i].name, end, need);
  }
}

}  // namespace

int main() {
  static_assert(CSM_MRL_MAX == 8, "UR_MRL_MAX_DIMS");
  const std::vector<std::vector<int32_t>> dim_sets = {{4},        {264},          {8, 16},          {8, 256, 264},           {64, 128, 256, 512, 1024},
                                                      {248, 1032}, {1024, 2048}, {4, 8, 12, 16, 20, 24, 28, 2048}};
  const char* slab_names[CSM_MRL_MAX] = {"slabs0", "slabs1", "slabs2", "slabs3", "slabs4", "slabs5", "slabs6", "slabs7"};
  long cases = 0;
  for (int32_t B : {0, 1, 3, 17, 33, 64, 512, 2000})
    for (int64_t N : {(int64_t)1, (int64_t)1023, (int64_t)1500, (int64_t)5003, (int64_t)1 << 20, (int64_t)INT32_MAX})
      for (int64_t chunk_rows : {(int64_t)0, (int64_t)1024, (int64_t)3072, (int64_t)1 << 18})
        for (const auto& dims : dim_sets)
          for (int grad = 0; grad < 2; ++grad) {
            const int K = (int)dims.size();
            // rows: the caller's figure, or the K planes together near 64 MB; at most N rounded up to 1024, at least one tile
            const int64_t n_up = cdiv(N, 1024) * 1024;
            int64_t rows = chunk_rows > 0 ? chunk_rows : ((int64_t)64 << 20) / (4 * (int64_t)std::max(B, 1) * K) / 1024 * 1024;
            rows = std::max<int64_t>(std::min(rows, n_up), 1024);
            const catalog_mrl_softmax_plan p = catalog_mrl_softmax_layout(B, N, K, dims.data(), chunk_rows, grad != 0);
            if (p.rows != rows || (p.rows % 1024) != 0) fail("chunk rows", "rows", p.rows, rows);
            if (chunk_rows == 0 && rows > 1024 && rows < n_up && (int64_t)K * std::max(B, 1) * rows * 4 > ((int64_t)64 << 20))
              fail("the planes exceed the chunk buffer", "rows", rows, K);
            if (p.seg != (int)cdiv(rows, CSM_SEGS)) fail("segment size", "seg", p.seg, rows);
            const int64_t vec = (int64_t)K * B * 4, run = (int64_t)K * B * CSM_SEGS * 4, chunk = (int64_t)K * B * rows * 4;
            std::vector<region> r = {{"chunk", p.chunk, chunk}, {"inv_u", p.inv_u, vec}, {"ref", p.ref, vec},
                                     {"m_run", p.m_run, run},   {"l_run", p.l_run, run}, {"t_run", p.t_run, run}};
            int64_t want = pad16(chunk) + 2 * pad16(vec) + 3 * pad16(run);
            for (int k = 0; k < K; ++k) {
              // what ur_catalog_softmax takes on the slice [:, :dims[k]] at the same rows
              int nsplit = 0, rps = 0;
              catalog_softmax_splits(B, dims[k], rows, &nsplit, &rps);
              if (p.nsplit[k] != nsplit || p.rps[k] != rps) fail("row splits", slab_names[k], p.nsplit[k], nsplit);
              if (rps % 4 != 0 || (int64_t)nsplit * rps < rows || (int64_t)(nsplit - 1) * rps >= rows) fail("splits do not cover the rows", slab_names[k], nsplit, rps);
              if (chunk_rows > 0) {
                const catalog_softmax_plan s = catalog_softmax_layout(B, N, dims[k], chunk_rows, grad != 0);
                if (s.rows != p.rows || s.seg != p.seg || s.nsplit != p.nsplit[k] || s.rps != p.rps[k]) fail("plane differs from the sliced call's plan", slab_names[k], s.rows, p.rows);
              }
              const int64_t slab = grad ? (int64_t)nsplit * B * dims[k] * 4 : 0;
              if (grad) r.push_back({slab_names[k], p.slabs[k], slab});
              want += pad16(slab);
            }
            check(p.need, std::max<int64_t>(16, want), r);
            ++cases;
          }
  std::printf("ok %ld\n", cases);
  return 0;
}
