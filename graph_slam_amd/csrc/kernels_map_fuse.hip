// Voxel-grid map fusion of depth frames on the MI355X (gfx950, f64 + 64-bit integers, wave64): the last stage of the reference's run,
// mapping/mapping_PCD.cpp:86-167 and mapping_PCD_rs.cpp:127-252 -- generatePointCloud, passThroughZ, Pw2c = Pw2j * Pu2c, the append
// to the map and pcl::VoxelGrid -- for ALL key frames in one call.  include/fgo.h states the semantics (this project's: a world-aligned
// grid, ONE centroid per voxel over all points of all frames, integer sums), tests/map_fuse_reference.py restates them in numpy.
//
//   points    a point costs a handful of flops: every product, quotient and sum of its arithmetic is rounded on its own (contraction
//             is switched off for those lines), the world coordinate is quantised to 2^-20 m and split into a voxel index and a
//             remainder by integer floor division (map_cells_device.hpp, as is the key).  From there on everything is integer.
//   table     ONE device-wide open-addressing hash table of 64-byte slots {key, n, S_x, S_y, S_z, C_0, C_1, C_2}, all 64-bit; the
//             empty key is all-ones, probing is linear and wraps at the end.  A slot is claimed by a 64-bit atomicCAS on its key and
//             summed into by 64-bit integer atomicAdd: the sums do not depend on the order of arrival.
//   insert    a workgroup takes a tile of MF_TILE sampled pixels and pre-aggregates it in an open-addressing table in LDS (MF_LDS =
//             2 MF_TILE slots, so it cannot fill; 64-bit CAS on the key, 64-bit adds on S, 32-bit adds on n and C, which a tile
//             cannot overflow); one lane per occupied LDS slot then claims the voxel's slot in the device-wide table and adds the
//             tile's partial sums.  What a tile IS decides what the LDS stage takes off the device-wide atomics.  `frames` (the
//             default, k_map_insert<true, 128>): a run of 4 sampled pixels in 128 consecutive frames -- along a trajectory the same
//             pixel of neighbouring frames looks at the same few voxels.  `lds` (<true, 1>): a run of 512 sampled pixels of ONE frame
//             -- at skip 2 and a 2 cm leaf neighbouring samples are 1.6 cm apart at 2 m, and 1.08 points share a slot.  `plain`
//             (<false, 1>): every point straight to the device-wide table.  The map does not depend on the form, nor on the order
//             of the frames; the time does.  FGO_MAP_INSERT=frames / lds / plain picks the form of a call (development; the
//             figures of all three: profiles/NOTES.md).
//   pack      the occupied slots with n >= min_points are compacted into (key, slot) pairs; the radix sort of map_cell_index.hip
//             orders the pairs over the 63 key bits; the keys are distinct, so the order does not depend on how the compaction went.
//   finalise  one thread per output row gathers centroid, colour, count and key through the sorted slots.
// No floating-point atomics anywhere.  Every barrier is outside every branch that is not uniform over the workgroup: the tile loop
// and its bounds are uniform, the point loop and the probe loops hold no barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/fgo.h"
#include "batch_call.hpp"
#include "map_cell_index.hpp"
#include "map_cells_device.hpp"

namespace fgo {
namespace {

using dev::MAP_CELL_BIAS, dev::MAP_CELL_EMPTY, dev::MAP_QUANTA_PER_M;      // |i_k| < 2^20; the key of no voxel; 2^20
constexpr int MF_T = 256;                        // threads of a workgroup
constexpr int MF_TILE = 512;                     // sampled pixels of a tile
constexpr int MF_LDS = 2 * MF_TILE;              // slots of the LDS table: at least twice the tile's points
constexpr int MF_MAX_PIXELS = 1 << 24;

struct MfSlot { unsigned long long key, n, s[3], c[3]; };      // 64 bytes

enum { MF_C_OOR = 0, MF_C_FULL = 1, MF_C_VOXELS = 2, MF_C_DROPPED = 3, MF_C_FRAMES = 4 };      // the counters; then one per frame

struct MfArgs {
  int64_t n_frames, ns, n_tiles;                 // sampled pixels of a frame, tiles of the call
  int W, H, ch, su, sv, sw, skip;
  int64_t tiles;                                 // tiles of a group of frames
  const uint16_t *depth;
  const uint8_t *color;
  const double *rt;                              // n x 12
  double fx, fy, cx, cy, z_scale, z_min, z_max;
  long long L;
  MfSlot *tab;
  unsigned long long mask;                       // 2^T - 1
  unsigned long long *counters;
};

__device__ inline unsigned long long mf_hash(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  return k ^ (k >> 33);
}

// one pixel: 0 = not valid, 1 = stored (key, r), 2 = out of range
__device__ inline int mf_point(const MfArgs &A, const double *__restrict__ rt, int u, int v, uint16_t w, unsigned long long &key, long long r[3]) {
#pragma clang fp contract(off)
  const double z = (double)w * A.z_scale;
  if (!(z > A.z_min && z < A.z_max)) return 0;
  const double p0 = (((double)u - A.cx) * z) / A.fx, p1 = (((double)v - A.cy) * z) / A.fy;
  long long i[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double x = ((rt[3 * k] * p0 + rt[3 * k + 1] * p1) + rt[3 * k + 2] * z) + rt[9 + k];
    long long Q;
    if (!dev::map_quantise(x, 0x1p62, Q)) return 2;            // not finite, or beyond any index (2^62)
    const long long q = dev::map_floor_div(Q, A.L);
    if (q <= -MAP_CELL_BIAS || q >= MAP_CELL_BIAS) return 2;
    i[k] = q;
    r[k] = Q - q * A.L;
  }
  key = dev::map_cell_key(i[0] + MAP_CELL_BIAS, i[1] + MAP_CELL_BIAS, i[2] + MAP_CELL_BIAS);
  return 1;
}

// claims the voxel's slot in the device-wide table and adds n, S and C; a probe that goes round the whole table raises FULL
__device__ inline void mf_global_add(const MfArgs &A, unsigned long long key, unsigned long long n, const unsigned long long s[3],
                                     const unsigned long long c[3]) {
  unsigned long long h = mf_hash(key) & A.mask;
  for (unsigned long long probes = 0; probes <= A.mask; ++probes, h = (h + 1) & A.mask) {
    MfSlot *e = A.tab + h;
    unsigned long long prev = __atomic_load_n(&e->key, __ATOMIC_RELAXED);      // a key, once written, stays
    if (prev != key) {
      if (prev != MAP_CELL_EMPTY) continue;
      prev = atomicCAS(&e->key, MAP_CELL_EMPTY, key);
      if (prev != MAP_CELL_EMPTY && prev != key) continue;
    }
    atomicAdd(&e->n, n);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (s[k]) atomicAdd(&e->s[k], s[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < A.ch && c[k]) atomicAdd(&e->c[k], c[k]);
    return;
  }
  A.counters[MF_C_FULL] = 1;                     // every lane that gets here stores the same value
}

__global__ __launch_bounds__(256) void k_map_init(MfSlot *tab, unsigned long long n_slots) {
  ulonglong2 *p = reinterpret_cast<ulonglong2 *>(tab);                         // four 16-byte pieces per slot; the first holds the key
  const unsigned long long n = 4 * n_slots, stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride)
    p[k] = make_ulonglong2((k & 3) == 0 ? MAP_CELL_EMPTY : 0ull, 0ull);
}

// A tile is PX = MF_TILE / FR consecutive sampled pixels of FR consecutive frames: FR = 1 is a run of one frame, FR > 1 the same run
// of pixels seen from a group of frames, which along a trajectory look at the same voxels.
template <bool AGG, int FR>
__global__ __launch_bounds__(MF_T) void k_map_insert(MfArgs A) {
  constexpr int PX = MF_TILE / FR;
  __shared__ unsigned long long s_key[AGG ? MF_LDS : 1];
  __shared__ unsigned long long s_sum[AGG ? 3 * MF_LDS : 1];
  __shared__ unsigned int s_cnt[AGG ? 4 * MF_LDS : 1];                         // n, C_0, C_1, C_2
  __shared__ unsigned int s_tot[FR + 1];                                       // the valid points of the tile's frames, its out-of-range points
  const int tid = threadIdx.x;
  const int64_t NP = (int64_t)A.W * A.H;
  for (int64_t b = blockIdx.x; b < A.n_tiles; b += gridDim.x) {                // uniform over the workgroup
    const int64_t g = b / A.tiles;                                             // the group of frames, the run of pixels
    const int64_t s0 = (b - g * A.tiles) * PX;
    if (AGG) {
      for (int s = tid; s < MF_LDS; s += MF_T) {
        s_key[s] = MAP_CELL_EMPTY;
        s_sum[3 * s] = s_sum[3 * s + 1] = s_sum[3 * s + 2] = 0;
        s_cnt[4 * s] = s_cnt[4 * s + 1] = s_cnt[4 * s + 2] = s_cnt[4 * s + 3] = 0;
      }
    }
    if (tid <= FR) s_tot[tid] = 0;
    __syncthreads();
    unsigned int n_oor = 0;
    for (int k = tid; k < MF_TILE; k += MF_T) {
      const int fr = k / PX;
      const int64_t f = g * FR + fr, s = s0 + (k - fr * PX);
      if (f >= A.n_frames || s >= A.ns) continue;
      const int row = (int)(s / A.sw), a = (int)(s - (int64_t)row * A.sw);
      const int u = A.su + a * A.skip, v = A.sv + row * A.skip;
      const int64_t pix = f * NP + (int64_t)v * A.W + u;
      unsigned long long key;
      long long r[3];
      const int st = mf_point(A, A.rt + 12 * f, u, v, A.depth[pix], key, r);
      n_oor += st == 2;
      if (st != 1) continue;
      atomicAdd(&s_tot[fr], 1u);
      unsigned int c[3] = {0, 0, 0};
      for (int k2 = 0; k2 < A.ch; ++k2) c[k2] = A.color[pix * A.ch + k2];
      if (AGG) {
        unsigned int h = (unsigned int)(mf_hash(key) >> 32) & (MF_LDS - 1);
        for (;;) {                                                             // ends: the tile has at most MF_LDS / 2 keys
          const unsigned long long prev = atomicCAS(&s_key[h], MAP_CELL_EMPTY, key);
          if (prev == MAP_CELL_EMPTY || prev == key) break;
          h = (h + 1) & (MF_LDS - 1);
        }
        atomicAdd(&s_cnt[4 * h], 1u);
#pragma unroll
        for (int k2 = 0; k2 < 3; ++k2) atomicAdd(&s_sum[3 * h + k2], (unsigned long long)r[k2]);
        for (int k2 = 0; k2 < A.ch; ++k2) atomicAdd(&s_cnt[4 * h + 1 + k2], c[k2]);
      } else {
        const unsigned long long s3[3] = {(unsigned long long)r[0], (unsigned long long)r[1], (unsigned long long)r[2]};
        const unsigned long long c3[3] = {c[0], c[1], c[2]};
        mf_global_add(A, key, 1ull, s3, c3);
      }
    }
    if (n_oor) atomicAdd(&s_tot[FR], n_oor);
    __syncthreads();
    if (AGG) {
      for (int s = tid; s < MF_LDS; s += MF_T) {
        const unsigned long long key = s_key[s];
        if (key == MAP_CELL_EMPTY) continue;
        const unsigned long long s3[3] = {s_sum[3 * s], s_sum[3 * s + 1], s_sum[3 * s + 2]};
        const unsigned long long c3[3] = {s_cnt[4 * s + 1], s_cnt[4 * s + 2], s_cnt[4 * s + 3]};
        mf_global_add(A, key, s_cnt[4 * s], s3, c3);
      }
    }
    if (tid < FR && g * FR + tid < A.n_frames && s_tot[tid])
      atomicAdd(&A.counters[MF_C_FRAMES + g * FR + tid], (unsigned long long)s_tot[tid]);
    if (tid == FR && s_tot[FR]) atomicAdd(&A.counters[MF_C_OOR], (unsigned long long)s_tot[FR]);
    __syncthreads();                                                           // the next tile clears the LDS table
  }
}

// the occupied slots with n >= min_points as (key, slot) pairs, in no particular order; the others are counted
__global__ __launch_bounds__(256) void k_map_pack(const MfSlot *__restrict__ tab, unsigned long long n_slots, unsigned long long min_points,
                                                  unsigned long long *counters, unsigned long long *pk, uint32_t *ps) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += stride) {
    const unsigned long long key = tab[s].key;
    if (key == MAP_CELL_EMPTY) continue;
    if (tab[s].n >= min_points) {
      const unsigned long long at = atomicAdd(&counters[MF_C_VOXELS], 1ull);
      pk[at] = key;
      ps[at] = (uint32_t)s;
    } else atomicAdd(&counters[MF_C_DROPPED], 1ull);
  }
}

__global__ __launch_bounds__(256) void k_map_finalise(const MfSlot *__restrict__ tab, const uint32_t *__restrict__ slot, int64_t m, long long L,
                                                      int ch, double *__restrict__ xyz, uint8_t *__restrict__ color,
                                                      int32_t *__restrict__ count, int64_t *__restrict__ key_out) {
#pragma clang fp contract(off)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
    const MfSlot e = tab[slot[j]];
    const double n = (double)e.n;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      xyz[3 * j + k] = ((double)((dev::map_cell_coord(e.key, k) - MAP_CELL_BIAS) * L) + (double)e.s[k] / n) * (1.0 / MAP_QUANTA_PER_M);
    for (int k = 0; k < ch; ++k) color[j * ch + k] = (uint8_t)((2 * e.c[k] + e.n) / (2 * e.n));
    count[j] = (int32_t)e.n;
    key_out[j] = (int64_t)e.key;
  }
}

// FGO_MAP_INSERT=plain / lds / frames: the insert form of a call (development).  The default is the form that measured fastest.
enum { MF_PLAIN, MF_LDS_FRAME, MF_LDS_GROUP };
constexpr int MF_GROUP = 128;                    // frames of a tile in the `frames` form: 4 pixels of 128 frames
int insert_form() {
  const char *e = std::getenv("FGO_MAP_INSERT");
  if (e && std::strcmp(e, "plain") == 0) return MF_PLAIN;
  if (e && std::strcmp(e, "lds") == 0) return MF_LDS_FRAME;
  if (e && std::strcmp(e, "frames") == 0) return MF_LDS_GROUP;
  return MF_LDS_GROUP;
}

double g_mf_kernel_ms = 0.0;

}  // namespace
}  // namespace fgo

extern "C" double fgo_debug_map_fuse_kernel_ms(void) { return fgo::g_mf_kernel_ms; }

extern "C" void fgo_map_params_default(fgo_map_params *p) {
  if (!p) return;
  p->fx = p->fy = 250.5773;
  p->cx = 90.0; p->cy = 70.0;
  p->z_scale = 0.001;
  p->z_min = 0.1; p->z_max = 5.0;
  p->skip = 2;
  p->rect[0] = p->rect[1] = p->rect[2] = p->rect[3] = 0;
  p->leaf = 0.02;
  p->min_points = 1;
  p->table_log2 = 0;
}

extern "C" int fgo_map_fuse_batch(int device, int64_t n_frames, int width, int height, const uint16_t *depth, const uint8_t *color, int channels,
                                  const double *pose_w7, const double *extrinsic7, const fgo_map_params *params, int64_t max_voxels,
                                  fgo_map_result *result, double *xyz_out, uint8_t *color_out, int32_t *count_out, int64_t *key_out,
                                  int64_t *frame_points_out, double *rt_out) {
  using namespace fgo;
  fgo_map_params P;
  fgo_map_params_default(&P);
  if (params) P = *params;
  if (!result || n_frames < 0 || max_voxels < 0) return FGO_EINVAL;
  if (width < 1 || height < 1 || (int64_t)width * height > MF_MAX_PIXELS) return FGO_EINVAL;
  if (channels != 0 && channels != 1 && channels != 3) return FGO_EINVAL;
  if (!pinhole_ok(P.fx, P.fy, P.cx, P.cy, P.z_scale) || !(P.z_min < P.z_max)) return FGO_EINVAL;
  if (P.skip < 1 || P.min_points < 1 || !in_closed(P.leaf, 1.0 / MAP_QUANTA_PER_M, 1024.0)) return FGO_EINVAL;
  if (P.table_log2 != 0 && (P.table_log2 < 4 || P.table_log2 > 32)) return FGO_EINVAL;
  int su = P.rect[0], sv = P.rect[1], eu = P.rect[2], ev = P.rect[3];
  if (su == 0 && sv == 0 && eu == 0 && ev == 0) { eu = width; ev = height; }
  if (su < 0 || sv < 0 || su >= eu || sv >= ev || eu > width || ev > height) return FGO_EINVAL;
  const int64_t sw = (eu - su + P.skip - 1) / P.skip, sh = (ev - sv + P.skip - 1) / P.skip, ns = sw * sh;
  if (n_frames > INT64_MAX / ns || n_frames * ns >= (1ll << 31)) return FGO_EINVAL;
  const int64_t n_sampled = n_frames * ns;
  std::memset(result, 0, sizeof *result);
  if (n_frames == 0) return FGO_OK;
  if (!depth || !pose_w7 || (color == nullptr) != (channels == 0) || (max_voxels > 0 && !xyz_out)) return FGO_EINVAL;
  std::vector<double> rt;
  if (!poses_rt(pose_w7, n_frames, extrinsic7, rt)) return FGO_EINVAL;
  if (int rc = select_device(device)) return rc;

  int T = P.table_log2;
  if (T == 0)
    for (T = 4; (1ll << T) < 2 * n_sampled; ++T) {}
  const unsigned long long n_slots = 1ull << T;
  const long long L = llrint(P.leaf * MAP_QUANTA_PER_M);
  result->table_log2 = T;
  result->n_sampled = n_sampled;

  // the frames; the table, the counters and the (key, slot) pairs of the pack: at most min(slots, sampled pixels) voxels
  const size_t nf = (size_t)n_frames, np = (size_t)width * (size_t)height, n_count = MF_C_FRAMES + nf;
  const size_t cap = (size_t)(n_slots < (unsigned long long)n_sampled ? n_slots : (unsigned long long)n_sampled);
  Staged S;
  const int h_depth = S.in(depth, nf * np * sizeof(uint16_t)), h_color = S.in(color, nf * np * (size_t)channels);
  const int h_rt = S.in(rt.data(), rt.size() * sizeof(double));
  const int h_tab = S.out(nullptr, (size_t)n_slots * sizeof(MfSlot), true), h_cnt = S.out(nullptr, n_count * sizeof(unsigned long long), true);
  const int h_pk = S.out(nullptr, cap * sizeof(unsigned long long), true), h_ps = S.out(nullptr, cap * sizeof(uint32_t), true);
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  unsigned long long *d_cnt = S.ptr<unsigned long long>(h_cnt);
  if (hipMemset(d_cnt, 0, n_count * sizeof(unsigned long long)) != hipSuccess) return FGO_ENUM;
  MfArgs A;
  const int form = insert_form(), fr = form == MF_LDS_GROUP ? MF_GROUP : 1, px = MF_TILE / fr;
  A.n_frames = n_frames; A.ns = ns; A.tiles = (ns + px - 1) / px; A.n_tiles = ((n_frames + fr - 1) / fr) * A.tiles;
  A.W = width; A.H = height; A.ch = channels; A.su = su; A.sv = sv; A.sw = (int)sw; A.skip = P.skip;
  A.depth = S.ptr<uint16_t>(h_depth); A.color = S.ptr<uint8_t>(h_color); A.rt = S.ptr<double>(h_rt);
  A.fx = P.fx; A.fy = P.fy; A.cx = P.cx; A.cy = P.cy; A.z_scale = P.z_scale; A.z_min = P.z_min; A.z_max = P.z_max;
  A.L = L; A.tab = S.ptr<MfSlot>(h_tab); A.mask = n_slots - 1; A.counters = d_cnt;
  KernelTimer timer1, timer2;                    // the table up to the pack; the sort and the output rows
  if (!timer1.start()) return FGO_ENUM;
  hipLaunchKernelGGL(k_map_init, dim3(grid_for(4 * n_slots, 256 * 8)), dim3(256), 0, 0, A.tab, n_slots);
  const dim3 grid(grid_for((unsigned long long)A.n_tiles, 1));
  if (form == MF_LDS_GROUP) hipLaunchKernelGGL((k_map_insert<true, MF_GROUP>), grid, dim3(MF_T), 0, 0, A);
  else if (form == MF_LDS_FRAME) hipLaunchKernelGGL((k_map_insert<true, 1>), grid, dim3(MF_T), 0, 0, A);
  else hipLaunchKernelGGL((k_map_insert<false, 1>), grid, dim3(MF_T), 0, 0, A);
  hipLaunchKernelGGL(k_map_pack, dim3(grid_for(n_slots, 256 * 4)), dim3(256), 0, 0, A.tab, n_slots, (unsigned long long)P.min_points, d_cnt,
                     S.ptr<unsigned long long>(h_pk), S.ptr<uint32_t>(h_ps));
  timer1.stop();
  std::vector<unsigned long long> cnt(n_count);
  if (hipMemcpy(cnt.data(), d_cnt, n_count * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess)
    return FGO_ENUM;
  g_mf_kernel_ms = timer1.ms();
  for (size_t f = 0; f < nf; ++f) {
    result->n_valid += (int64_t)cnt[MF_C_FRAMES + f];
    if (frame_points_out) frame_points_out[f] = (int64_t)cnt[MF_C_FRAMES + f];
  }
  result->n_out_of_range = (int64_t)cnt[MF_C_OOR];
  if (rt_out) std::memcpy(rt_out, rt.data(), rt.size() * sizeof(double));
  if (cnt[MF_C_FULL]) {
    result->status = FGO_MAP_FULL;
    return FGO_OK;
  }
  const size_t nv = (size_t)cnt[MF_C_VOXELS], m = nv < (size_t)max_voxels ? nv : (size_t)max_voxels;
  result->n_voxels = (int64_t)nv;
  result->n_dropped = (int64_t)cnt[MF_C_DROPPED];
  result->status = m < nv ? FGO_MAP_TRUNCATED : FGO_MAP_OK;
  if (m == 0) return FGO_OK;

  // the sorted pairs, the sort's scratch and the m output rows: sized now that the number of voxels is known
  size_t tmp_bytes = 0;
  if (int rc = map_sort_pairs_bytes(nv, 63, tmp_bytes)) return rc;
  Arena B;
  const size_t o_tmp = B.reserve(tmp_bytes), o_sk = B.reserve(nv * sizeof(unsigned long long)), o_ss = B.reserve(nv * sizeof(uint32_t));
  const size_t o_xyz = B.reserve(3 * m * sizeof(double)), o_col = B.reserve(m * (size_t)channels), o_n = B.reserve(m * sizeof(int32_t));
  const size_t o_key = B.reserve(m * sizeof(int64_t));
  if (B.alloc() != hipSuccess) return FGO_ENOMEM;
  if (!timer2.start()) return FGO_ENUM;
  if (int rc = map_sort_pairs(B.at<void>(o_tmp), tmp_bytes, S.ptr<unsigned long long>(h_pk), B.at<unsigned long long>(o_sk), S.ptr<uint32_t>(h_ps),
                              B.at<uint32_t>(o_ss), nv, 63))
    return rc;
  hipLaunchKernelGGL(k_map_finalise, dim3(grid_for(m, 256)), dim3(256), 0, 0, A.tab, B.at<uint32_t>(o_ss), (int64_t)m, L, channels,
                     B.at<double>(o_xyz), B.at<uint8_t>(o_col), B.at<int32_t>(o_n), B.at<int64_t>(o_key));
  timer2.stop();
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  g_mf_kernel_ms += timer2.ms();
  // only the m rows go back
  void *const host[4] = {xyz_out, channels ? color_out : nullptr, count_out, key_out};
  const size_t off[4] = {o_xyz, o_col, o_n, o_key}, bytes[4] = {3 * m * sizeof(double), m * (size_t)channels, m * sizeof(int32_t), m * sizeof(int64_t)};
  for (int k = 0; k < 4; ++k)
    if (host[k] && bytes[k] && hipMemcpy(host[k], B.at<char>(off[k]), bytes[k], hipMemcpyDeviceToHost) != hipSuccess) return FGO_ENUM;
  return FGO_OK;
}
