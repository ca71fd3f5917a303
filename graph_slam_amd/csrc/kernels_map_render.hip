// Z-buffer rendering of the map from trajectory poses on the MI355X (gfx950, f64 + 64-bit integers, wave64): what the reference's
// mapping/map_video*.cpp do with a VTK viewer, frame after frame -- place a camera relative to the sensor (map_video.cpp:119-127,187),
// draw the accumulated map from there, fly an arc round it (:210-238) -- for ALL views in one call, and the map's self-check: the map
// drawn from a key frame's own camera predicts that frame's depth image.  include/fgo.h states the semantics (this project's: a
// point is a square of pixels, a pixel keeps the minimum of the 64-bit word (zq << 32) | index over the points that cover it),
// tests/map_render_reference.py restates them in numpy.
//
//   point     one lane projects one point into one view: every product, quotient and sum is rounded on its own (contraction is off
//             for the whole file), the depth is quantised to 2^-20 m, the footprint is clipped to the image.  From there on
//             everything is integer; a minimum does not depend on the order of arrival.
//   tiles     (the form FGO_MAP_RENDER=tiles) the grid is (row strips of the image) x views.  A workgroup of 256 lanes owns one
//             strip of one view in an LDS z-buffer of MR_STRIP = 8192 words = 64 KiB (two workgroups share a CU's 160 KiB); a strip
//             is tile_rows = max(1, 8192 / width) rows.  The workgroup walks the WHOLE cloud in chunks of 256 consecutive points,
//             clips each footprint to its strip and issues one 64-bit atomicMin on LDS (ds_min_u64) per covered pixel; after one
//             barrier the lanes resolve the strip.  No global z-buffer, no init pass, no device-wide atomics on pixels; the price
//             is that every strip of a view projects every point again.  An image wider than 8192 pixels does not fit a strip
//             row: such a call runs in the global form, whatever FGO_MAP_RENDER says (result.form tells).
//   global    (FGO_MAP_RENDER=global) k_render_init sets a device z-buffer of views x H x W words to all ones, k_render_points
//             projects every (view, point) once and issues device-wide 64-bit atomicMins, k_render_resolve does what the strip
//             resolve does.  A z-buffer above MR_ZWORDS words is not allocated: the VIEWS are then taken in chunks (views do not
//             share pixels, so the outputs do not depend on the chunking).
//   resolve   zq, index and colour are written coalesced, the colour gathered through the winner's index; the depth check runs
//             against the measured words; the counts are reduced in the workgroup (wave shuffles, then LDS) and added with one
//             integer atomic per counter per workgroup.  n_valid, n_drawn and n_nonfinite are properties of a point, not of a
//             strip: in the tiles form only the workgroup of strip 0 (and for n_nonfinite of view 0) counts them.
// The 12 numbers of a view are uniform over the workgroup.  No floating-point atomics anywhere.  Every barrier is outside every
// branch that is not uniform over the workgroup: the tile loops and their bounds are uniform, the point loop holds no barrier.
// The quantum is the map's (map_cells_device.hpp); the host side shares the checks of camera and poses with the fusion (batch_call.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/fgo.h"
#include "batch_call.hpp"
#include "map_cells_device.hpp"

#pragma clang fp contract(off)

namespace fgo {
namespace {

using dev::MAP_QUANTA_PER_M;                     // depths are quantised to the map's quantum, 2^-20 m
constexpr int MR_T = 256;                        // threads of a workgroup
constexpr int MR_STRIP = 8192;                   // pixels of a strip: 64 KiB of 64-bit words
constexpr int MR_MAX_PIXELS = 1 << 24;
constexpr int MR_MAX_HALF = 32;
constexpr unsigned long long MR_EMPTY = ~0ull;
constexpr unsigned long long MR_ZWORDS = 1ull << 27;       // the global form's z-buffer holds at most this many words (1 GiB)

// the counters of a workgroup: the eight of fgo_map_render_view in its order, then the call's n_nonfinite
enum { MR_C_VALID, MR_C_DRAWN, MR_C_PIXELS, MR_C_MEAS, MR_C_BOTH, MR_C_AGREE, MR_C_CLOSER, MR_C_THROUGH, MR_C_NONFINITE, MR_NC };
constexpr int MR_VIEW_COUNTS = 8;

struct MrArgs {
  int64_t n_points, n_views, view0;              // the views of this launch are view0 .. view0 + n_views - 1
  int W, H, ch, tile_rows, n_strips;
  const double *xyz;
  const uint8_t *color;
  const double *rt;                              // all views x 12
  const uint16_t *depth;                         // all views x H x W, or NULL
  double fx, fy, cx, cy, z_scale, z_min, z_max, radius;
  int splat, max_half;
  long long tq;
  unsigned char bg[3];
  unsigned long long *zbuf;                      // global form: n_views x H x W words
  unsigned long long *counts;                    // all views x 8
  unsigned long long *nonfinite;                 // 1
  int32_t *zq_out, *index_out;                   // all views x H x W, or NULL
  uint8_t *color_out;                            // all views x H x W x ch, or NULL
};

enum { MR_P_NONFINITE = 0, MR_P_INVALID = 1, MR_P_VALID = 2, MR_P_DRAWN = 3 };
struct MrFoot { int u_lo, u_hi, v_lo, v_hi, zq; };         // the footprint clipped to the image, bounds included

// one point in one view (rt uniform over the workgroup): what became of it, and for MR_P_DRAWN its depth and footprint
__device__ inline int mr_project(const MrArgs &A, const double (&rt)[12], int64_t i, MrFoot &f) {
  const double x0 = A.xyz[3 * i], x1 = A.xyz[3 * i + 1], x2 = A.xyz[3 * i + 2];
  if (!(fabs(x0) < HUGE_VAL && fabs(x1) < HUGE_VAL && fabs(x2) < HUGE_VAL)) return MR_P_NONFINITE;
  const double d0 = x0 - rt[9], d1 = x1 - rt[10], d2 = x2 - rt[11];
  const double p0 = (rt[0] * d0 + rt[3] * d1) + rt[6] * d2, p1 = (rt[1] * d0 + rt[4] * d1) + rt[7] * d2;
  const double z = (rt[2] * d0 + rt[5] * d1) + rt[8] * d2;
  if (!(z > A.z_min && z < A.z_max)) return MR_P_INVALID;
  f.zq = (int)llrint(z * MAP_QUANTA_PER_M);            // 0 <= zq < 2^31: z_max <= 2047
  const double uf = ((A.fx * p0) / z) + A.cx, vf = ((A.fy * p1) / z) + A.cy;
  const double B = 1073741824.0;                 // 2^30
  if (!(uf > -B && uf < B && vf > -B && vf < B)) return MR_P_VALID;          // off-image, NaN included
  const int u0 = (int)floor(uf + 0.5), v0 = (int)floor(vf + 0.5);
  int h = A.splat;
  if (A.radius > 0) {
    const double s = floor((A.fx * A.radius) / z);                           // >= 0, may be +inf
    h = s >= (double)A.max_half ? A.max_half : A.splat + (int)s;
  }
  if (h > A.max_half) h = A.max_half;
  f.u_lo = max(u0 - h, 0); f.u_hi = min(u0 + h, A.W - 1);
  f.v_lo = max(v0 - h, 0); f.v_hi = min(v0 + h, A.H - 1);
  return f.u_lo <= f.u_hi && f.v_lo <= f.v_hi ? MR_P_DRAWN : MR_P_VALID;
}

__device__ inline unsigned long long mr_word(int zq, int64_t i) { return ((unsigned long long)(unsigned)zq << 32) | (unsigned long long)(unsigned)i; }

// one pixel of one view from its word: the outputs the caller asked for, and the lane's counts
__device__ inline void mr_resolve(const MrArgs &A, int64_t view, int64_t pix, unsigned long long word, unsigned (&c)[MR_NC]) {
  const bool covered = word != MR_EMPTY;
  const int zq = covered ? (int)(word >> 32) : -1, index = covered ? (int)(unsigned)word : -1;
  const int64_t o = view * ((int64_t)A.W * A.H) + pix;
  if (A.zq_out) A.zq_out[o] = zq;
  if (A.index_out) A.index_out[o] = index;
  if (A.color_out)
    for (int k = 0; k < A.ch; ++k) A.color_out[o * A.ch + k] = covered ? A.color[(int64_t)index * A.ch + k] : A.bg[k];
  c[MR_C_PIXELS] += covered;
  if (!A.depth) return;
  const double zm = (double)A.depth[o] * A.z_scale;
  if (!(zm > A.z_min && zm < A.z_max)) return;
  c[MR_C_MEAS] += 1;
  if (!covered) return;
  const long long d = llrint(zm * MAP_QUANTA_PER_M) - (long long)zq;
  c[MR_C_BOTH] += 1;
  c[MR_C_AGREE] += d <= A.tq && d >= -A.tq;
  c[MR_C_CLOSER] += d < -A.tq;
  c[MR_C_THROUGH] += d > A.tq;
}

// Adds the workgroup's counts to the view's counters (and n_nonfinite to the call's): a wave reduces by shuffles, the four waves
// through s_red (4 MR_NC words), one atomic per non-zero counter.  Every lane of the workgroup calls it; the caller has a barrier
// between the last use of s_red's memory and this call, and the call ends with one.
__device__ inline void mr_block_add(const MrArgs &A, int64_t view, unsigned (&c)[MR_NC], unsigned *s_red) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < MR_NC; ++k)
    for (int off = 32; off > 0; off >>= 1) c[k] += __shfl_down(c[k], off);
  if ((tid & 63) == 0)
    for (int k = 0; k < MR_NC; ++k) s_red[(tid >> 6) * MR_NC + k] = c[k];
  __syncthreads();
  if (tid < MR_NC) {
    const unsigned s = (s_red[tid] + s_red[MR_NC + tid]) + (s_red[2 * MR_NC + tid] + s_red[3 * MR_NC + tid]);
    if (s) atomicAdd(tid < MR_VIEW_COUNTS ? &A.counts[MR_VIEW_COUNTS * view + tid] : A.nonfinite, (unsigned long long)s);
  }
  __syncthreads();
}

__global__ __launch_bounds__(MR_T) void k_render_tiles(MrArgs A) {
  __shared__ unsigned long long s_z[MR_STRIP];
  const int tid = threadIdx.x;
  const int64_t n_tiles = A.n_views * A.n_strips;
  for (int64_t b = blockIdx.x; b < n_tiles; b += gridDim.x) {                  // uniform over the workgroup
    const int64_t view = A.view0 + b / A.n_strips;
    const int strip = (int)(b % A.n_strips);
    const int row0 = strip * A.tile_rows, rows = min(A.tile_rows, A.H - row0), npx = rows * A.W;      // npx <= MR_STRIP
    for (int p = tid; p < npx; p += MR_T) s_z[p] = MR_EMPTY;
    double rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) rt[k] = A.rt[12 * view + k];
    unsigned c[MR_NC];
#pragma unroll
    for (int k = 0; k < MR_NC; ++k) c[k] = 0;
    __syncthreads();
    for (int64_t base = 0; base < A.n_points; base += MR_T) {                  // no barrier inside
      const int64_t i = base + tid;
      if (i >= A.n_points) continue;
      MrFoot f;
      const int st = mr_project(A, rt, i, f);
      if (strip == 0) {
        c[MR_C_NONFINITE] += st == MR_P_NONFINITE && view == 0;
        c[MR_C_VALID] += st >= MR_P_VALID;
        c[MR_C_DRAWN] += st == MR_P_DRAWN;
      }
      if (st != MR_P_DRAWN) continue;
      const int v_lo = max(f.v_lo, row0), v_hi = min(f.v_hi, row0 + rows - 1);
      const unsigned long long word = mr_word(f.zq, i);
      for (int v = v_lo; v <= v_hi; ++v)
        for (int u = f.u_lo; u <= f.u_hi; ++u) atomicMin(&s_z[(v - row0) * A.W + u], word);
    }
    __syncthreads();
    for (int p = tid; p < npx; p += MR_T) mr_resolve(A, view, (int64_t)row0 * A.W + p, s_z[p], c);
    __syncthreads();                                                           // the z-buffer is read: its memory serves the reduction
    mr_block_add(A, view, c, reinterpret_cast<unsigned *>(s_z));               // ends with a barrier: the next tile clears the z-buffer
  }
}

__global__ __launch_bounds__(256) void k_render_init(unsigned long long *zbuf, unsigned long long n) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) zbuf[k] = MR_EMPTY;
}

// a tile is 256 consecutive points of one view
__global__ __launch_bounds__(MR_T) void k_render_points(MrArgs A) {
  __shared__ unsigned s_red[4 * MR_NC];
  const int tid = threadIdx.x;
  const int64_t NP = (int64_t)A.W * A.H, per_view = (A.n_points + MR_T - 1) / MR_T, n_tiles = A.n_views * per_view;
  for (int64_t b = blockIdx.x; b < n_tiles; b += gridDim.x) {                  // uniform over the workgroup
    const int64_t lv = b / per_view, view = A.view0 + lv, i = (b % per_view) * MR_T + tid;
    double rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) rt[k] = A.rt[12 * view + k];
    unsigned c[MR_NC];
#pragma unroll
    for (int k = 0; k < MR_NC; ++k) c[k] = 0;
    if (i < A.n_points) {
      MrFoot f;
      const int st = mr_project(A, rt, i, f);
      c[MR_C_NONFINITE] += st == MR_P_NONFINITE && view == 0;
      c[MR_C_VALID] += st >= MR_P_VALID;
      c[MR_C_DRAWN] += st == MR_P_DRAWN;
      if (st == MR_P_DRAWN) {
        const unsigned long long word = mr_word(f.zq, i);
        unsigned long long *z = A.zbuf + lv * NP;
        for (int v = f.v_lo; v <= f.v_hi; ++v)
          for (int u = f.u_lo; u <= f.u_hi; ++u) atomicMin(&z[(int64_t)v * A.W + u], word);
      }
    }
    mr_block_add(A, view, c, s_red);
  }
}

// a tile is 256 consecutive pixels of one view
__global__ __launch_bounds__(MR_T) void k_render_resolve(MrArgs A) {
  __shared__ unsigned s_red[4 * MR_NC];
  const int tid = threadIdx.x;
  const int64_t NP = (int64_t)A.W * A.H, per_view = (NP + MR_T - 1) / MR_T, n_tiles = A.n_views * per_view;
  for (int64_t b = blockIdx.x; b < n_tiles; b += gridDim.x) {                  // uniform over the workgroup
    const int64_t lv = b / per_view, view = A.view0 + lv, pix = (b % per_view) * MR_T + tid;
    unsigned c[MR_NC];
#pragma unroll
    for (int k = 0; k < MR_NC; ++k) c[k] = 0;
    if (pix < NP) mr_resolve(A, view, pix, A.zbuf[lv * NP + pix], c);
    mr_block_add(A, view, c, s_red);
  }
}

// FGO_MAP_RENDER=tiles / global: the kernel form of a call (development).  The default is the form that measured faster.
int render_form() {
  const char *e = std::getenv("FGO_MAP_RENDER");
  if (e && std::strcmp(e, "tiles") == 0) return FGO_MAP_RENDER_TILES;
  if (e && std::strcmp(e, "global") == 0) return FGO_MAP_RENDER_GLOBAL;
  return FGO_MAP_RENDER_TILES;
}

// FGO_MAP_RENDER_ZWORDS: the words of the global form's z-buffer (development: lets a small call take its views in chunks)
unsigned long long zbuf_words() {
  const char *e = std::getenv("FGO_MAP_RENDER_ZWORDS");
  const long long v = e ? std::atoll(e) : 0;
  return v > 0 ? (unsigned long long)v : MR_ZWORDS;
}

bool length_ok(double v) { return v >= 0 && v <= 2047.0; }          // false for NaN

double g_mr_kernel_ms = 0.0;

}  // namespace
}  // namespace fgo

extern "C" double fgo_debug_map_render_kernel_ms(void) { return fgo::g_mr_kernel_ms; }

extern "C" void fgo_map_render_params_default(fgo_map_render_params *p) {
  if (!p) return;
  p->fx = p->fy = 250.5773;
  p->cx = 90.0; p->cy = 70.0;
  p->z_scale = 0.001;
  p->z_min = 0.1; p->z_max = 50.0;
  p->splat = 0;
  p->radius = 0.0;
  p->max_half = 8;
  p->agree_tol = 0.05;
  p->background[0] = 0; p->background[1] = 0; p->background[2] = 26;
}

extern "C" int fgo_map_render_batch(int device, int64_t n_points, const double *xyz, const uint8_t *color, int channels, int64_t n_views,
                                    const double *pose_w7, const double *extrinsic7, const double *view_offset7, int width, int height,
                                    const fgo_map_render_params *params, const uint16_t *depth_meas, fgo_map_render_result *result,
                                    fgo_map_render_view *view_out, int32_t *zq_out, int32_t *index_out, uint8_t *color_out, double *rt_out) {
  using namespace fgo;
  fgo_map_render_params P;
  fgo_map_render_params_default(&P);
  if (params) P = *params;
  if (!result || n_points < 0 || n_views < 0 || n_points >= (1ll << 31)) return FGO_EINVAL;
  if (width < 1 || height < 1 || (int64_t)width * height > MR_MAX_PIXELS) return FGO_EINVAL;
  const int64_t NP = (int64_t)width * height;
  if (n_views > INT64_MAX / NP || n_views * NP >= (1ll << 31)) return FGO_EINVAL;
  if (channels != 0 && channels != 1 && channels != 3) return FGO_EINVAL;
  if (!pinhole_ok(P.fx, P.fy, P.cx, P.cy, P.z_scale)) return FGO_EINVAL;
  if (!(P.z_min >= 0) || !(P.z_max <= 2047.0) || !(P.z_min < P.z_max)) return FGO_EINVAL;
  if (P.splat < 0 || P.splat > MR_MAX_HALF || P.max_half < P.splat || P.max_half > MR_MAX_HALF) return FGO_EINVAL;
  if (!length_ok(P.radius) || !length_ok(P.agree_tol)) return FGO_EINVAL;
  if (color_out && channels == 0) return FGO_EINVAL;
  if (n_views > 0 && !pose_w7) return FGO_EINVAL;
  if (n_points > 0 && (!xyz || (color == nullptr) != (channels == 0))) return FGO_EINVAL;
  std::vector<double> rt;
  if ((view_offset7 && !quat_ok(view_offset7 + 3)) || !poses_rt(pose_w7, n_views, extrinsic7, rt)) return FGO_EINVAL;
  std::memset(result, 0, sizeof *result);
  if (n_views == 0) return FGO_OK;
  if (int rc = select_device(device)) return rc;

  const size_t nv = (size_t)n_views, np = (size_t)NP, n = (size_t)n_points;
  if (view_offset7) {                                                          // the view: the sensor with the offset composed on the right
    const std::vector<double> rt1 = rt;
    for (size_t v = 0; v < nv; ++v) rt_compose(rt1.data() + 12 * v, view_offset7, rt.data() + 12 * v);
  }
  int form = render_form();
  if (width > MR_STRIP) form = FGO_MAP_RENDER_GLOBAL;                          // a row does not fit a strip
  const unsigned long long zcap = zbuf_words();
  const int64_t chunk = form == FGO_MAP_RENDER_GLOBAL ? (int64_t)(zcap / np < 1 ? 1 : zcap / np < nv ? zcap / np : nv) : 0;

  Staged S;
  const int h_xyz = S.in(xyz, 3 * n * sizeof(double)), h_color = S.in(n ? color : nullptr, n * (size_t)channels);
  const int h_rt = S.in(rt.data(), rt.size() * sizeof(double)), h_depth = S.in(depth_meas, nv * np * sizeof(uint16_t));
  const size_t n_count = MR_VIEW_COUNTS * nv + 1;
  const int h_cnt = S.out(nullptr, n_count * sizeof(unsigned long long), true);
  const int h_zbuf = S.out(nullptr, (size_t)chunk * np * sizeof(unsigned long long), chunk > 0);
  const int h_zq = S.out(zq_out, nv * np * sizeof(int32_t)), h_index = S.out(index_out, nv * np * sizeof(int32_t));
  const int h_cout = S.out(color_out, nv * np * (size_t)channels);
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  unsigned long long *d_cnt = S.ptr<unsigned long long>(h_cnt);
  if (hipMemset(d_cnt, 0, n_count * sizeof(unsigned long long)) != hipSuccess) return FGO_ENUM;

  MrArgs A;
  A.n_points = n_points; A.n_views = n_views; A.view0 = 0;
  A.W = width; A.H = height; A.ch = channels;
  A.tile_rows = form == FGO_MAP_RENDER_TILES ? (MR_STRIP / width > 1 ? MR_STRIP / width : 1) : 0;
  A.n_strips = form == FGO_MAP_RENDER_TILES ? (height + A.tile_rows - 1) / A.tile_rows : 0;
  A.xyz = S.ptr<double>(h_xyz); A.color = S.ptr<uint8_t>(h_color); A.rt = S.ptr<double>(h_rt); A.depth = S.ptr<uint16_t>(h_depth);
  A.fx = P.fx; A.fy = P.fy; A.cx = P.cx; A.cy = P.cy; A.z_scale = P.z_scale; A.z_min = P.z_min; A.z_max = P.z_max; A.radius = P.radius;
  A.splat = P.splat; A.max_half = P.max_half; A.tq = llrint(P.agree_tol * MAP_QUANTA_PER_M);
  for (int k = 0; k < 3; ++k) A.bg[k] = P.background[k];
  A.zbuf = chunk > 0 ? S.ptr<unsigned long long>(h_zbuf) : nullptr;
  A.counts = d_cnt; A.nonfinite = d_cnt + MR_VIEW_COUNTS * nv;
  A.zq_out = S.ptr<int32_t>(h_zq); A.index_out = S.ptr<int32_t>(h_index); A.color_out = S.ptr<uint8_t>(h_cout);

  KernelTimer timer;
  if (!timer.start()) return FGO_ENUM;
  if (form == FGO_MAP_RENDER_TILES) {
    hipLaunchKernelGGL(k_render_tiles, dim3(grid_for(n_views * A.n_strips, 1)), dim3(MR_T), 0, 0, A);
  } else {
    for (int64_t v0 = 0; v0 < n_views; v0 += chunk) {                          // the views in chunks: they share no pixel
      A.view0 = v0; A.n_views = n_views - v0 < chunk ? n_views - v0 : chunk;
      const unsigned long long words = (unsigned long long)A.n_views * np;
      hipLaunchKernelGGL(k_render_init, dim3(grid_for(words, 256 * 8)), dim3(256), 0, 0, A.zbuf, words);
      if (n_points > 0)
        hipLaunchKernelGGL(k_render_points, dim3(grid_for(A.n_views * ((n_points + MR_T - 1) / MR_T), 1)), dim3(MR_T), 0, 0, A);
      hipLaunchKernelGGL(k_render_resolve, dim3(grid_for(A.n_views * ((NP + MR_T - 1) / MR_T), 1)), dim3(MR_T), 0, 0, A);
    }
  }
  timer.stop();
  std::vector<unsigned long long> cnt(n_count);
  if (hipMemcpy(cnt.data(), d_cnt, n_count * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess)
    return FGO_ENUM;
  g_mr_kernel_ms = timer.ms();
  if (int rc = S.download()) return rc;
  if (view_out)
    for (size_t v = 0; v < nv; ++v) {
      const unsigned long long *c = cnt.data() + MR_VIEW_COUNTS * v;
      fgo_map_render_view &o = view_out[v];
      o.n_valid = (int64_t)c[MR_C_VALID]; o.n_drawn = (int64_t)c[MR_C_DRAWN]; o.n_pixels = (int64_t)c[MR_C_PIXELS];
      o.n_meas = (int64_t)c[MR_C_MEAS]; o.n_both = (int64_t)c[MR_C_BOTH]; o.n_agree = (int64_t)c[MR_C_AGREE];
      o.n_closer = (int64_t)c[MR_C_CLOSER]; o.n_through = (int64_t)c[MR_C_THROUGH];
    }
  if (rt_out) std::memcpy(rt_out, rt.data(), rt.size() * sizeof(double));
  result->n_points = n_points;
  result->n_nonfinite = (int64_t)cnt[MR_VIEW_COUNTS * nv];
  result->form = form;
  result->tile_rows = A.tile_rows;
  return FGO_OK;
}
