// Host-only check of the catalogue workspaces (unirec_amd/csrc/catalog_layout.hip.h), built with -fsanitize=address,undefined by
// tests/test_catalog_select_host.py.  Over a grid of sizes, for every entry point: each region starts on a 16-byte boundary, no two
// regions overlap, the last one ends inside `need`, and `need` is the closed form the host tests pin (written out here a second time,
// from the documented layout and not from the carver).  Exit status 0 and "ok <cases>" on success.
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
  std::fprintf(stderr, "catalog_layout_check: %s: %s %s (%lld, %lld)\n", entry, what, name, a, b);
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
  const int64_t N = (int64_t)1 << 30;            // large enough that chunk_rows is taken as given
  long cases = 0;
  for (int32_t B : {0, 1, 3, 17, 512, 2000})
    for (int64_t rows : {(int64_t)1024, (int64_t)2048, (int64_t)1 << 18})
      for (int32_t K : {1, 129, 1024})
        for (int32_t D : {4, 40, 1024, 2048})
          for (int32_t segments : {0, 1, 16}) {
            const int64_t chunk = (int64_t)B * rows * 4, vec = (int64_t)B * 4;
            if (catalog_chunk_rows(rows, B, N) != rows) fail("chunk rows", "catalog_chunk_rows", "", rows, B);

            const select_plan s = select_layout(B, N, rows);
            check("select", s.need, std::max<int64_t>(16, pad16(chunk) + pad16(vec)), {{"chunk", s.chunk, chunk}, {"ref", s.ref, vec}});

            const int gw = segments > 0 ? segments : (int)std::min<int64_t>(std::max<int64_t>(1024 / std::max(B, 1), 1), 8);
            const int64_t list = (int64_t)B * gw * K * 4, count = (int64_t)B * gw * 4;
            const deep_plan d = deep_layout(B, N, K, rows, segments);
            if (d.gw != gw) fail("segments", "deep", "gw", d.gw, gw);
            check("deep", d.need, std::max<int64_t>(16, pad16(chunk) + 2 * pad16(vec) + 2 * pad16(list) + pad16(count)),
                  {{"chunk", d.chunk, chunk}, {"ref", d.ref, vec}, {"inv_u", d.inv_u, vec}, {"list_score", d.list_score, list},
                   {"list_index", d.list_index, list}, {"count", d.count, count}});

            const coarse_plan c = coarse_layout(B, N, D, rows);
            const int64_t ubf = (int64_t)B * D * 2;
            check("coarse", c.need, std::max<int64_t>(16, pad16(ubf) + 2 * pad16(vec) + pad16(chunk)),
                  {{"user", c.user, ubf}, {"inv_u", c.inv_u, vec}, {"ref", c.ref, vec}, {"chunk", c.chunk, chunk}});

            // the softmax slabs: ~1024 workgroups of 32 users x 256 columns in all, no split shorter than 64 rows, rows per split % 4 == 0
            const int64_t tiles = cdiv(std::max(B, 1), 32) * cdiv(D, 256);
            const int64_t splits = std::max<int64_t>(1, std::min<int64_t>(1024 / tiles, cdiv(rows, 64)));
            const int64_t rps = cdiv(cdiv(rows, splits), 4) * 4, nsplit = cdiv(rows, rps);
            const int64_t seg = (int64_t)B * 16 * 4;
            for (bool grad : {false, true}) {
              const int64_t slabs = grad ? nsplit * B * D * 4 : 0;
              const catalog_softmax_plan m = catalog_softmax_layout(B, N, D, rows, grad);
              if (m.nsplit != nsplit || m.rps != rps) fail("splits", "softmax", "nsplit", m.nsplit, nsplit);
              check("softmax", m.need, std::max<int64_t>(16, pad16(chunk) + 2 * pad16(vec) + 3 * seg + slabs),
                    {{"chunk", m.chunk, chunk}, {"inv_u", m.inv_u, vec}, {"ref", m.ref, vec}, {"m_run", m.m_run, seg}, {"l_run", m.l_run, seg},
                     {"t_run", m.t_run, seg}, {"slabs", m.slabs, slabs}});
            }
            ++cases;
          }
  std::printf("ok %ld\n", cases);
  return 0;
}
