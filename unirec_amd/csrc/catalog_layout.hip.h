// The workspaces of the catalogue entry points, each described once: a layout function carves the regions with ws_carver and records
// their offsets in its plan, the size query answers the carver's final position, and the launches take their pointers from the same
// offsets -- the size and the carving cannot disagree.  Plain C++ with no HIP header, so that a host program can include it
// (tests/host/catalog_layout_check.cpp); the constants here are the ones the sizes depend on.
#pragma once
#include <cstdint>

namespace {

constexpr int SEL_TILE = 1024;                 // scores per sweep step of the selection kernels: 4 per thread
constexpr int CSM_SEGS = 16;                   // workgroups per user's chunk row in the softmax fold and weight kernels
constexpr int CSM_UT = 2, CSM_USERS = 16 * CSM_UT;      // user tiles and users of a workgroup of the softmax gradient kernel
// workgroups per user's chunk row the deep selection may choose by itself (catalog_deep.hip.h, deep_segments)
constexpr int DEEP_SEGMENTS_AUTO = 8;

// take(bytes): the offset of the next region; every region starts on a 16-byte boundary
struct ws_carver {
  int64_t pos = 0;
  int64_t take(int64_t bytes) {
    const int64_t at = pos;
    pos += (bytes + 15) / 16 * 16;
    return at;
  }
  int64_t need() const { return pos > 16 ? pos : 16; }
};

// rows per chunk of the streaming mode: the caller's figure, or a chunk buffer [B, rows] near 64 MB (so that it can stay in the
// Infinity Cache between the scoring and the selection launch); never more than N rounded up to the selection tile
static int64_t catalog_chunk_rows(int64_t chunk_rows, int32_t B, int64_t N) {
  const int64_t n_up = (N + SEL_TILE - 1) / SEL_TILE * SEL_TILE;
  int64_t r = chunk_rows;
  if (r <= 0) r = ((int64_t)64 << 20) / (4 * (int64_t)(B > 0 ? B : 1)) / SEL_TILE * SEL_TILE;
  if (r > n_up) r = n_up;
  if (r > ((int64_t)1 << 30)) r = (int64_t)1 << 30;           // the selection kernel indexes a chunk with an int
  if (r < SEL_TILE) r = SEL_TILE;
  return r;
}

// ur_catalog_scores, select mode: chunk [B][rows] f32 | ref [B]
struct select_plan {
  int64_t rows, chunk, ref, need;
};
static select_plan select_layout(int32_t B, int64_t N, int64_t chunk_rows) {
  select_plan p;
  ws_carver c;
  p.rows = catalog_chunk_rows(chunk_rows, B, N);
  p.chunk = c.take((int64_t)B * p.rows * 4);
  p.ref = c.take((int64_t)B * 4);
  p.need = c.need();
  return p;
}

// ur_catalog_deep_select: chunk [B][rows] f32 | ref [B] | inv_u [B] | list scores [B][gw][K] | list indices [B][gw][K] | counts [B][gw].
// gw = the workgroups per user's chunk row the workspace is laid out for (sizes alone: the size query touches no device); the launch
// takes no more (deep_segments).
static int deep_segments_cap(int32_t segments, int32_t B) {
  if (segments > 0) return segments;
  int g = 1024 / (B > 0 ? B : 1);
  return g < 1 ? 1 : g > DEEP_SEGMENTS_AUTO ? DEEP_SEGMENTS_AUTO : g;
}
struct deep_plan {
  int64_t rows, chunk, ref, inv_u, list_score, list_index, count, need;
  int gw;
};
static deep_plan deep_layout(int32_t B, int64_t N, int32_t K, int64_t chunk_rows, int32_t segments) {
  deep_plan p;
  ws_carver c;
  p.rows = catalog_chunk_rows(chunk_rows, B, N);
  p.gw = deep_segments_cap(segments, B);
  p.chunk = c.take((int64_t)B * p.rows * 4);
  p.ref = c.take((int64_t)B * 4);
  p.inv_u = c.take((int64_t)B * 4);
  p.list_score = c.take((int64_t)B * p.gw * K * 4);
  p.list_index = c.take((int64_t)B * p.gw * K * 4);
  p.count = c.take((int64_t)B * p.gw * 4);
  p.need = c.need();
  return p;
}

// ur_catalog_softmax: chunk [B][rows] | inv_u [B] | ref [B] | m, l, t: [B][CSM_SEGS] each | slabs [nsplit][B][D] (with d_user only).
// Row splits of the gradient product: ~1024 workgroups in all, no split shorter than 64 rows; rps = rows per split (a multiple of 4).
static void catalog_softmax_splits(int32_t B, int32_t D, int64_t rows, int* nsplit, int* rps) {
  const long tiles = (long)(((B > 0 ? B : 1) + CSM_USERS - 1) / CSM_USERS) * ((D + 255) / 256);
  long s = 1024 / tiles;
  if (s > (rows + 63) / 64) s = (rows + 63) / 64;
  if (s < 1) s = 1;
  long r = ((rows + s - 1) / s + 3) / 4 * 4;
  *rps = (int)r;
  *nsplit = (int)((rows + r - 1) / r);
}
struct catalog_softmax_plan {
  int64_t rows, chunk, inv_u, ref, m_run, l_run, t_run, slabs, need;
  int nsplit, rps, seg;
};
static catalog_softmax_plan catalog_softmax_layout(int32_t B, int64_t N, int32_t D, int64_t chunk_rows, bool grad) {
  catalog_softmax_plan p;
  ws_carver c;
  p.rows = catalog_chunk_rows(chunk_rows, B, N);
  p.seg = (int)((p.rows + CSM_SEGS - 1) / CSM_SEGS);
  catalog_softmax_splits(B, D, p.rows, &p.nsplit, &p.rps);
  p.chunk = c.take((int64_t)B * p.rows * 4);
  p.inv_u = c.take((int64_t)B * 4);
  p.ref = c.take((int64_t)B * 4);
  p.m_run = c.take((int64_t)B * CSM_SEGS * 4);
  p.l_run = c.take((int64_t)B * CSM_SEGS * 4);
  p.t_run = c.take((int64_t)B * CSM_SEGS * 4);
  p.slabs = c.take(grad ? (int64_t)p.nsplit * B * D * 4 : 0);      // (no d_user: no pass 2, nothing reads the offset)
  p.need = c.need();
  return p;
}

// ur_catalog_mrl_softmax (include/unirec_hip_mrl_loss.h): K planes of the plan above, plane k at width dims[k], sharing the chunk rows:
// scores [K][B][rows] | inv_u [K][B] | ref [K][B] | m, l, t: [K][B][CSM_SEGS] each | per plane: slabs [nsplit_k][B][d_k] (with d_user only).
// rows, left to the library: the K planes together near 64 MB.  seg is the one of the chunk rows and (nsplit_k, rps_k) are
// catalog_softmax_splits(B, d_k, rows): what ur_catalog_softmax takes on the slice at the same chunk_rows.
constexpr int CSM_MRL_MAX = 8;                 // = UR_MRL_MAX_DIMS (include/unirec_hip_mrl.h)
static int64_t catalog_mrl_chunk_rows(int64_t chunk_rows, int32_t B, int64_t N, int32_t K) {
  if (chunk_rows > 0) return catalog_chunk_rows(chunk_rows, B, N);
  const int64_t r = ((int64_t)64 << 20) / (4 * (int64_t)(B > 0 ? B : 1) * (K > 0 ? K : 1)) / SEL_TILE * SEL_TILE;
  return catalog_chunk_rows(r < SEL_TILE ? SEL_TILE : r, B, N);
}
struct catalog_mrl_softmax_plan {
  int64_t rows, chunk, inv_u, ref, m_run, l_run, t_run, slabs[CSM_MRL_MAX], need;
  int nsplit[CSM_MRL_MAX], rps[CSM_MRL_MAX], seg;
};
[[maybe_unused]] static catalog_mrl_softmax_plan catalog_mrl_softmax_layout(int32_t B, int64_t N, int32_t K, const int32_t* dims, int64_t chunk_rows,
                                                                             bool grad) {
  catalog_mrl_softmax_plan p{};
  ws_carver c;
  p.rows = catalog_mrl_chunk_rows(chunk_rows, B, N, K);
  p.seg = (int)((p.rows + CSM_SEGS - 1) / CSM_SEGS);
  p.chunk = c.take((int64_t)K * B * p.rows * 4);
  p.inv_u = c.take((int64_t)K * B * 4);
  p.ref = c.take((int64_t)K * B * 4);
  p.m_run = c.take((int64_t)K * B * CSM_SEGS * 4);
  p.l_run = c.take((int64_t)K * B * CSM_SEGS * 4);
  p.t_run = c.take((int64_t)K * B * CSM_SEGS * 4);
  for (int k = 0; k < K; ++k) {
    catalog_softmax_splits(B, dims[k], p.rows, &p.nsplit[k], &p.rps[k]);
    p.slabs[k] = c.take(grad ? (int64_t)p.nsplit[k] * B * dims[k] * 4 : 0);      // (no d_user: no pass 2, nothing reads the offsets)
  }
  p.need = c.need();
  return p;
}

// ur_catalog_coarse_select: u~ [B][D] bf16 | iu~ [B] | ref [B] | chunk [B][rows] f32
struct coarse_plan {
  int64_t rows, user, inv_u, ref, chunk, need;
};
static coarse_plan coarse_layout(int32_t B, int64_t N, int32_t D, int64_t chunk_rows) {
  coarse_plan p;
  ws_carver c;
  p.rows = catalog_chunk_rows(chunk_rows, B, N);
  p.user = c.take((int64_t)B * D * 2);
  p.inv_u = c.take((int64_t)B * 4);
  p.ref = c.take((int64_t)B * 4);
  p.chunk = c.take((int64_t)B * p.rows * 4);
  p.need = c.need();
  return p;
}

// ur_catalog_coarse_deep_select: the coarse pass's regions, then the deep selection's lists:
// u~ [B][D] bf16 | iu~ [B] | ref [B] | chunk [B][rows] f32 | list scores [B][gw][K] | list indices [B][gw][K] | counts [B][gw]
struct coarse_deep_plan {
  int64_t rows, user, inv_u, ref, chunk, list_score, list_index, count, need;
  int gw;
};
[[maybe_unused]] static coarse_deep_plan coarse_deep_layout(int32_t B, int64_t N, int32_t D, int32_t K, int64_t chunk_rows, int32_t segments) {
  coarse_deep_plan p;
  ws_carver c;
  p.rows = catalog_chunk_rows(chunk_rows, B, N);
  p.gw = deep_segments_cap(segments, B);
  p.user = c.take((int64_t)B * D * 2);
  p.inv_u = c.take((int64_t)B * 4);
  p.ref = c.take((int64_t)B * 4);
  p.chunk = c.take((int64_t)B * p.rows * 4);
  p.list_score = c.take((int64_t)B * p.gw * K * 4);
  p.list_index = c.take((int64_t)B * p.gw * K * 4);
  p.count = c.take((int64_t)B * p.gw * 4);
  p.need = c.need();
  return p;
}

// ur_catalog_deep_rerank: iu [B] | scores [B][K_in] f32 (what the scoring launch hands the sorting one)
struct deep_rerank_plan {
  int64_t inv_u, score, need;
};
[[maybe_unused]] static deep_rerank_plan deep_rerank_layout(int32_t B, int32_t K_in) {
  deep_rerank_plan p;
  ws_carver c;
  p.inv_u = c.take((int64_t)B * 4);
  p.score = c.take((int64_t)B * K_in * 4);
  p.need = c.need();
  return p;
}

// ur_catalog_funnel_select / ur_catalog_funnel_rerank (include/unirec_hip_funnel.h): the two plans above at D = dim.  The staged user
// prefix is a contiguous [B][dim] block and the catalogue is read in place, so the strides ld / ldu size nothing.
[[maybe_unused]] static coarse_deep_plan funnel_select_layout(int32_t B, int64_t N, int32_t dim, int32_t K, int64_t chunk_rows, int32_t segments) {
  return coarse_deep_layout(B, N, dim, K, chunk_rows, segments);
}
[[maybe_unused]] static deep_rerank_plan funnel_rerank_layout(int32_t B, int32_t K_in) { return deep_rerank_layout(B, K_in); }

// ur_catalog_fp8_select (include/unirec_fp8.h): the quantised users, then the regions of the long coarse select:
// q [B][D] bytes | iu8 [B] | user scales [B] | ref [B] | chunk [B][rows] f32 | list scores [B][gw][K] | list indices [B][gw][K] | counts [B][gw]
struct fp8_select_plan {
  int64_t rows, user, inv_u, scale_u, ref, chunk, list_score, list_index, count, need;
  int gw;
};
[[maybe_unused]] static fp8_select_plan fp8_select_layout(int32_t B, int64_t N, int32_t D, int32_t K, int64_t chunk_rows, int32_t segments) {
  fp8_select_plan p;
  ws_carver c;
  p.rows = catalog_chunk_rows(chunk_rows, B, N);
  p.gw = deep_segments_cap(segments, B);
  p.user = c.take((int64_t)B * D);
  p.inv_u = c.take((int64_t)B * 4);
  p.scale_u = c.take((int64_t)B * 4);
  p.ref = c.take((int64_t)B * 4);
  p.chunk = c.take((int64_t)B * p.rows * 4);
  p.list_score = c.take((int64_t)B * p.gw * K * 4);
  p.list_index = c.take((int64_t)B * p.gw * K * 4);
  p.count = c.take((int64_t)B * p.gw * 4);
  p.need = c.need();
  return p;
}
// ur_catalog_fp8_rerank: the plan of ur_catalog_deep_rerank (the code rows are read in place)
[[maybe_unused]] static deep_rerank_plan fp8_rerank_layout(int32_t B, int32_t K_in) { return deep_rerank_layout(B, K_in); }

}  // namespace
