// Place recognition by visual words on the MI355X (gfx950, wave64): fgo_vocab_train and fgo_place_query_batch.  include/fgo_place.h
// states the semantics, tests/place_reference.py restates them in numpy.  The kernels:
//
//   k_place_norms   one thread per descriptor: |u - 128|^2 over its 128 bytes (<= 2^21).
//   k_place_assign  the hot path of both calls: the nearest centre of EVERY feature of the call.  The distance product is the one of
//                   kernels_feature_match.hip -- a byte u read as the int8 u ^ 0x80, d = |a'|^2 + |b'|^2 - 2 a'.b' with a'.b' on
//                   v_mfma_i32_16x16x64_i8, two K-steps per 16 x 16 tile; lane l holds bytes [64 s + 16 (l >> 4), + 16) of row (l & 15)
//                   in K-step s for A (features) and B (centres) alike; D: centre column l & 15, feature row 4 (l >> 4) + reg -- with
//                   features   blocks of PL_FB = 256: a wave owns four 16-feature strips whose A fragments, norms and running
//                              (d1, w1) stay in registers while the centres go by; a B fragment is read once for the four strips.
//                   centres    chunks of PL_TC = 128 staged in LDS (16 KB), 16-byte slot c of row r stored at slot c ^ (r & 7), and
//                              the chunk's norms (-1: a row past V).
//                   rows       a lane keeps (d1, w1) for its 4 rows of a strip; the centres reach it in ascending w, so a strict
//                              compare keeps the lowest index of a tie; the 16 lanes of a row merge after the last chunk by a
//                              butterfly on (d, w), compared lexicographically.  No second neighbour, no column minimum.
//   training        k_place_stats (per feature: the word's count, and per wave one atomic each for the changed-count and the inertia),
//                   k_place_sums (one thread per byte: an integer atomicAdd into V x 128 sums), k_place_update (the new centres).
//   k_place_hist    one workgroup per frame: V 16-bit counters in LDS (two to a 32-bit word, filled with 32-bit LDS atomics: a count
//                   is <= 4096, no carry crosses), df by integer global atomics, and a block scan that compacts the non-zero counts
//                   into the frame's (word, count) list in ascending word order, at most one entry per feature.
//   k_place_weigh   one wave per frame: count * weight in place of the count, and the frame's norm2 in int64.
//   k_place_score   one workgroup per query frame a: v[a] as a dense int32 table in LDS (4 V bytes), the waves stride over the
//                   database frames' lists and reduce int64 dots (every lane leaves its loop before the first shuffle).  A wave keeps
//                   its 64 best (s, b, dot) one per lane, sorted by (s descending, b ascending): an insertion is a ballot and a
//                   shift by one lane.  The order is total, so the list does not depend on the order of the insertions; wave 0
//                   merges the four lists through LDS (the table's, no longer needed) and writes the first top_k.
// No floating-point atomics; every barrier is under control flow that is uniform over the workgroup (the frame / block / chunk
// loops); no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include <cmath>
#include <vector>
#include "../../include/fgo_place.h"
#include "batch_call.hpp"

namespace fgo {
namespace {

constexpr int PL_T = 256, PL_WAVES = 4, PL_STRIPS = 4;      // threads, waves, 16-feature strips per wave
constexpr int PL_FB = 16 * PL_STRIPS * PL_WAVES;            // features per block: 256
constexpr int PL_TC = 128;                                  // centres per LDS chunk
constexpr int PL_NONE = INT_MAX;                            // "no distance": larger than any (<= 8 323 200)
constexpr int PL_K = 64;                                    // the candidates a wave keeps: top_k <= 64
constexpr int PL_MERGE_BYTES = (PL_WAVES - 1) * PL_K * 20;  // the lists of waves 1 .. 3: double, int64, int32 per entry
static_assert(PL_MERGE_BYTES % 16 == 0, "the merge area is carved into aligned arrays");

typedef int v4i __attribute__((ext_vector_type(4)));

// one thread per descriptor: |u - 128|^2 summed over the 128 bytes (<= 128 * 128^2 = 2^21)
__global__ __launch_bounds__(256) void k_place_norms(int64_t n, const uint8_t *__restrict__ desc, int32_t *__restrict__ nrm) {
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < n; f += (int64_t)gridDim.x * 256) {
    const uint4 *__restrict__ row = reinterpret_cast<const uint4 *>(desc + f * FGO_FM_DIM);
    int s = 0;
#pragma unroll
    for (int c = 0; c < FGO_FM_DIM / 16; ++c) {
      const uint4 w = row[c];
      const uint32_t v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int e = (int)((v[k] >> (8 * b)) & 255u) - 128;
          s += e * e;
        }
    }
    nrm[f] = s;
  }
}

__device__ inline v4i flip(uint4 w) {
  return v4i{(int)(w.x ^ 0x80808080u), (int)(w.y ^ 0x80808080u), (int)(w.z ^ 0x80808080u), (int)(w.w ^ 0x80808080u)};
}

__global__ __launch_bounds__(PL_T, 2) void k_place_assign(int64_t F, const uint8_t *__restrict__ desc, const int32_t *__restrict__ nrm, int V,
                                                          const uint8_t *__restrict__ cen, const int32_t *__restrict__ cnrm,
                                                          int32_t *__restrict__ word, int32_t *__restrict__ word_d) {
  __shared__ __attribute__((aligned(16))) uint8_t s_cen[PL_TC * FGO_FM_DIM];       // the centre chunk, slots swizzled
  __shared__ int s_nb[PL_TC];                                                      // centre norms of the chunk, -1: past V
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lg = lane >> 4;
  const int64_t n_blocks = (F + PL_FB - 1) / PL_FB;
  const int n_chunks = (V + PL_TC - 1) / PL_TC;
  for (int64_t fb = blockIdx.x; fb < n_blocks; fb += gridDim.x) {
    // ---- the wave's strips: A fragments, norms, and the running (d1, w1) of the lane's 4 rows
    const int64_t w0 = fb * PL_FB + wave * 16 * PL_STRIPS;   // first feature of the wave in this block
    v4i a0[PL_STRIPS], a1[PL_STRIPS];
    int na[PL_STRIPS][4], d1[PL_STRIPS][4], w1[PL_STRIPS][4];
#pragma unroll
    for (int s = 0; s < PL_STRIPS; ++s) {
      const int64_t a = w0 + 16 * s + lc;                    // the row this lane loads
      a0[s] = a1[s] = v4i{0, 0, 0, 0};
      if (a < F) {
        const uint4 *__restrict__ row = reinterpret_cast<const uint4 *>(desc + a * FGO_FM_DIM);
        a0[s] = flip(row[lg]);
        a1[s] = flip(row[4 + lg]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t ar = w0 + 16 * s + 4 * lg + r;         // the rows this lane receives
        na[s][r] = ar < F ? nrm[ar] : 0;
        d1[s][r] = PL_NONE; w1[s][r] = PL_NONE;
      }
    }

    for (int ch = 0; ch < n_chunks; ++ch) {
      const int c0 = ch * PL_TC;
      __syncthreads();                                       // the chunk before this one has been read
      // ---- stage: 1024 16-byte slots, four per thread; rows past V are zero
#pragma unroll
      for (int k = 0; k < PL_TC * 8 / PL_T; ++k) {
        const int slot = tid + k * PL_T, r = slot >> 3, c = slot & 7;
        v4i v = {0, 0, 0, 0};
        if (c0 + r < V) v = flip(reinterpret_cast<const uint4 *>(cen + (int64_t)(c0 + r) * FGO_FM_DIM)[c]);
        *reinterpret_cast<v4i *>(s_cen + r * FGO_FM_DIM + ((c ^ (r & 7)) << 4)) = v;
      }
      if (tid < PL_TC) s_nb[tid] = c0 + tid < V ? cnrm[c0 + tid] : -1;
      __syncthreads();

      const int n_tiles = w0 < F ? (min(V - c0, PL_TC) + 15) >> 4 : 0;       // uniform over the wave; no barrier below
      for (int tile = 0; tile < n_tiles; ++tile) {
        const int row = 16 * tile + lc;                      // the centre this lane loads and receives
        const v4i f0 = *reinterpret_cast<const v4i *>(s_cen + row * FGO_FM_DIM + ((lg ^ (row & 7)) << 4));
        const v4i f1 = *reinterpret_cast<const v4i *>(s_cen + row * FGO_FM_DIM + (((4 + lg) ^ (row & 7)) << 4));
        const int nb = s_nb[row], w = c0 + row;
#pragma unroll
        for (int s = 0; s < PL_STRIPS; ++s) {
          if (w0 + 16 * s >= F) continue;                    // uniform over the wave
          v4i acc = {0, 0, 0, 0};
          acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0[s], f0, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1[s], f1, acc, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r) {                      // strict compare: the centres come in ascending w
            const int d = nb >= 0 ? na[s][r] + nb - 2 * acc[r] : PL_NONE;
            const bool better = d < d1[s][r];
            w1[s][r] = better ? w : w1[s][r];
            d1[s][r] = better ? d : d1[s][r];
          }
        }
      }
    }

    // ---- merge the 16 lanes of a row: lexicographic (d, w); then lane 0 of the row group writes its 4 rows
#pragma unroll
    for (int s = 0; s < PL_STRIPS; ++s) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int x1 = d1[s][r], xw = w1[s][r];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
          const int y1 = __shfl_xor(x1, m), yw = __shfl_xor(xw, m);
          const bool other = y1 < x1 || (y1 == x1 && yw < xw);
          x1 = other ? y1 : x1;
          xw = other ? yw : xw;
        }
        const int64_t a = w0 + 16 * s + 4 * lg + r;
        if (lc == 0 && a < F) {
          word[a] = xw;
          word_d[a] = x1;
        }
      }
    }
  }
}

// ---- training ---------------------------------------------------------------------------------------------------------------------
// scal[0]: the features whose word is not prev's (prev == NULL: none is counted), scal[1]: the sum of d
__global__ __launch_bounds__(256) void k_place_stats(int64_t F, const int32_t *__restrict__ word, const int32_t *__restrict__ prev,
                                                     const int32_t *__restrict__ word_d, uint32_t *__restrict__ count,
                                                     unsigned long long *__restrict__ scal) {
  const int64_t span = ((F + 255) / 256 + gridDim.x - 1) / gridDim.x * 256;        // per workgroup, a multiple of 256: whole waves loop alike
  unsigned long long changed = 0, inertia = 0;
  for (int64_t k = threadIdx.x; k < span; k += 256) {
    const int64_t f = (int64_t)blockIdx.x * span + k;
    if (f < F) {
      const int w = word[f];
      atomicAdd(&count[w], 1u);
      changed += prev && prev[f] != w;
      inertia += (unsigned long long)word_d[f];
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    changed += __shfl_xor(changed, m);
    inertia += __shfl_xor(inertia, m);
  }
  if ((threadIdx.x & 63) == 0) {
    if (changed) atomicAdd(&scal[0], changed);
    if (inertia) atomicAdd(&scal[1], inertia);
  }
}

// one thread per byte of desc: F <= 2^24 members of 255 at the most fit 32 bits
__global__ __launch_bounds__(256) void k_place_sums(int64_t F, const uint8_t *__restrict__ desc, const int32_t *__restrict__ word,
                                                    uint32_t *__restrict__ sums) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < F * FGO_FM_DIM; i += (int64_t)gridDim.x * 256)
    atomicAdd(&sums[(int64_t)word[i >> 7] * FGO_FM_DIM + (i & 127)], (uint32_t)desc[i]);
}

// round half up in integers; a word without a member keeps its centre
__global__ __launch_bounds__(256) void k_place_update(int V, const uint32_t *__restrict__ sums, const uint32_t *__restrict__ count,
                                                      uint8_t *__restrict__ cen) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= V * FGO_FM_DIM) return;
  const unsigned long long n = count[i >> 7];
  if (n > 0) cen[i] = (uint8_t)((2ull * sums[i] + n) / (2ull * n));
}

// ---- the words of a frame -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PL_T) void k_place_hist(int64_t n_frames, const int64_t *__restrict__ feat_ptr, const int32_t *__restrict__ word,
                                                     int V, int32_t *__restrict__ lw, int32_t *__restrict__ lc, int32_t *__restrict__ ln,
                                                     int32_t *__restrict__ df) {
  __shared__ uint32_t s_cnt[FGO_PLACE_MAX_WORDS / 2];        // word w: bits [16 (w & 1), + 16) of s_cnt[w >> 1]
  __shared__ int s_scan[PL_T];
  const int tid = threadIdx.x;
  const int per = (V + PL_T - 1) / PL_T, lo = min(tid * per, V), hi = min(lo + per, V);     // the thread's words, ascending with tid
  for (int64_t n = blockIdx.x; n < n_frames; n += gridDim.x) {
    const int64_t f0 = feat_ptr[n], f1 = feat_ptr[n + 1];
    for (int i = tid; i < (V + 1) / 2; i += PL_T) s_cnt[i] = 0;
    __syncthreads();
    for (int64_t f = f0 + tid; f < f1; f += PL_T) {
      const int w = word[f];
      atomicAdd(&s_cnt[w >> 1], 1u << (16 * (w & 1)));
    }
    __syncthreads();
    int nz = 0;
    for (int w = lo; w < hi; ++w) nz += ((s_cnt[w >> 1] >> (16 * (w & 1))) & 0xffffu) != 0;
    s_scan[tid] = nz;
    __syncthreads();
    for (int off = 1; off < PL_T; off <<= 1) {               // inclusive scan; the trip count is fixed
      const int v = tid >= off ? s_scan[tid - off] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    int64_t pos = f0 + s_scan[tid] - nz;
    for (int w = lo; w < hi; ++w) {
      const int c = (int)((s_cnt[w >> 1] >> (16 * (w & 1))) & 0xffffu);
      if (c) {
        lw[pos] = w; lc[pos] = c; ++pos;
        atomicAdd(&df[w], 1);
      }
    }
    if (tid == 0) ln[n] = s_scan[PL_T - 1];
    __syncthreads();                                         // s_cnt and s_scan are read before the next frame clears them
  }
}

// one wave per frame: the list's counts become v = count * weight, norm2 = sum v^2
__global__ __launch_bounds__(256) void k_place_weigh(int64_t n_frames, const int64_t *__restrict__ feat_ptr, const int32_t *__restrict__ ln,
                                                     const int32_t *__restrict__ lw, int32_t *__restrict__ lv, const int32_t *__restrict__ q,
                                                     int64_t *__restrict__ norm2) {
  const int lane = threadIdx.x & 63;
  for (int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); n < n_frames; n += (int64_t)gridDim.x * 4) {
    const int64_t f0 = feat_ptr[n];
    const int len = ln[n];
    long long acc = 0;
    for (int e = lane; e < len; e += 64) {
      const int v = lv[f0 + e] * q[lw[f0 + e]];
      lv[f0 + e] = v;
      acc += (long long)v * v;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) norm2[n] = acc;
  }
}

// ---- scoring ------------------------------------------------------------------------------------------------------------------------
struct ScoreArgs {
  int64_t n_frames;
  const int64_t *feat_ptr, *norm2;
  const int32_t *ln, *lw, *lv;
  int V, top_k, min_gap;
  double min_score;
  int32_t *n_cand;
  int64_t *cand_frame, *cand_dot, *dot;                      // dot may be NULL
  double *cand_score;
};

// the wave's list, one entry per lane, sorted: (s, b, dot) goes in front of the first entry it beats, the entries behind move up a lane
__device__ inline void insert(int lane, double s, int b, long long dot, double &ms, int &mb, long long &md) {
  const bool ahead = ms > s || (ms == s && mb < b);          // an empty lane holds (-1, INT_MAX): behind everything
  const int pos = __popcll(__ballot(ahead));
  const double ps = __shfl_up(ms, 1);
  const int pb = __shfl_up(mb, 1);
  const long long pd = __shfl_up(md, 1);
  if (lane == pos) { ms = s; mb = b; md = dot; }
  else if (lane > pos) { ms = ps; mb = pb; md = pd; }
}

__global__ __launch_bounds__(PL_T) void k_place_score(ScoreArgs A) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];            // max(4 V, PL_MERGE_BYTES) bytes
  int32_t *s_v = reinterpret_cast<int32_t *>(s_mem);                               // v[a][.], dense
  double *m_s = reinterpret_cast<double *>(s_mem);                                 // afterwards: the lists of waves 1 .. 3
  long long *m_d = reinterpret_cast<long long *>(s_mem + (PL_WAVES - 1) * PL_K * 8);
  int *m_b = reinterpret_cast<int *>(s_mem + (PL_WAVES - 1) * PL_K * 16);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t a = blockIdx.x; a < A.n_frames; a += gridDim.x) {
    const int64_t last = a - A.min_gap;                      // the database: b <= last
    for (int w = tid; w < A.V; w += PL_T) s_v[w] = 0;
    __syncthreads();
    const int64_t fa = A.feat_ptr[a];
    for (int e = tid; e < A.ln[a]; e += PL_T) s_v[A.lw[fa + e]] = A.lv[fa + e];
    if (A.dot)
      for (int64_t b = max(last + 1, (int64_t)0) + tid; b < A.n_frames; b += PL_T) A.dot[a * A.n_frames + b] = -1;
    __syncthreads();

    const long long n2a = A.norm2[a];
    double ms = -1.0;
    int mb = INT_MAX;
    long long md = 0;
    for (int64_t b = wave; b <= last; b += PL_WAVES) {
      const int64_t fb = A.feat_ptr[b];
      const int len = A.ln[b];
      long long dot = 0;
      for (int e = lane; e < len; e += 64) dot += (long long)s_v[A.lw[fb + e]] * (long long)A.lv[fb + e];
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) dot += __shfl_xor(dot, m);                  // every lane has left the loop above
      if (A.dot && lane == 0) A.dot[a * A.n_frames + b] = dot;
      if (dot <= 0) continue;                                // uniform over the wave: dot > 0 has both norms > 0
      const double s = (double)dot / sqrt((double)n2a * (double)A.norm2[b]);
      if (!(s >= A.min_score)) continue;
      const double ts = __shfl(ms, A.top_k - 1);             // the entry a candidate has to beat (b is new: it never ties on both)
      if (!(s > ts)) continue;                               // b ascends within a wave: on equal scores the entry stays ahead
      insert(lane, s, (int)b, dot, ms, mb, md);
    }
    __syncthreads();                                         // the table has been read: its LDS takes the lists
    if (wave > 0) {
      const int at = (wave - 1) * PL_K + lane;
      m_s[at] = ms; m_d[at] = md; m_b[at] = mb;
    }
    __syncthreads();
    if (wave == 0) {
      for (int e = 0; e < (PL_WAVES - 1) * PL_K; ++e) {
        const double s = m_s[e];
        if ((e & (PL_K - 1)) >= A.top_k || s < 0) continue;  // past a wave's first top_k, or empty; uniform over the wave
        insert(lane, s, m_b[e], m_d[e], ms, mb, md);
      }
      const bool have = lane < A.top_k && ms >= 0;
      const int n = __popcll(__ballot(have));
      if (lane < A.top_k) {
        A.cand_frame[a * A.top_k + lane] = have ? mb : -1;
        A.cand_dot[a * A.top_k + lane] = have ? md : 0;
        A.cand_score[a * A.top_k + lane] = have ? ms : 0.0;
      }
      if (lane == 0 && A.n_cand) A.n_cand[a] = n;
    }
    __syncthreads();                                         // the lists have been read before the next frame's table
  }
}

double g_place_kernel_ms = 0.0, g_place_phase_ms[3] = {0.0, 0.0, 0.0};

bool vocab_size_ok(int V) { return V >= 1 && V <= FGO_PLACE_MAX_WORDS; }

// the norms of the features and of the centres, then the nearest centre of every feature
void launch_assign(int64_t F, const uint8_t *desc, int32_t *nrm, bool with_feature_norms, int V, const uint8_t *cen, int32_t *cnrm,
                   int32_t *word, int32_t *word_d) {
  if (F <= 0) return;
  if (with_feature_norms) hipLaunchKernelGGL(k_place_norms, dim3(grid_for((unsigned long long)F, 256)), dim3(256), 0, 0, F, desc, nrm);
  hipLaunchKernelGGL(k_place_norms, dim3(grid_for((unsigned long long)V, 256)), dim3(256), 0, 0, (int64_t)V, cen, cnrm);
  hipLaunchKernelGGL(k_place_assign, dim3(grid_for((unsigned long long)F, PL_FB)), dim3(PL_T), 0, 0, F, desc, nrm, V, cen, cnrm, word, word_d);
}

}  // namespace
}  // namespace fgo

extern "C" double fgo_debug_place_kernel_ms(void) { return fgo::g_place_kernel_ms; }

extern "C" void fgo_debug_place_phase_ms(double out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = fgo::g_place_phase_ms[k];
}

extern "C" void fgo_vocab_params_default(fgo_vocab_params *p) {
  if (!p) return;
  p->n_words = 1024;
  p->n_iters = 10;
}

extern "C" void fgo_place_params_default(fgo_place_params *p) {
  if (!p) return;
  p->top_k = 5;
  p->min_gap = 10;
  p->min_score = 0.0;
  p->max_df_permille = 1000;
}

extern "C" int fgo_vocab_train(int device, int64_t F, const uint8_t *desc, const fgo_vocab_params *params, uint8_t *centres_out,
                               int64_t *count_out, fgo_vocab_result *result) {
  using namespace fgo;
  fgo_vocab_params P;
  fgo_vocab_params_default(&P);
  if (params) P = *params;
  if (!desc || !centres_out || !count_out || !result) return FGO_EINVAL;
  if (!vocab_size_ok(P.n_words) || F < P.n_words || F > FGO_PLACE_MAX_TRAIN || P.n_iters < 0) return FGO_EINVAL;
  const int V = P.n_words;
  const size_t nf = (size_t)F, nv = (size_t)V, row = FGO_FM_DIM;
  for (int64_t w = 0; w < V; ++w) {                          // init: descriptor floor(w F / V)
    const uint8_t *src = desc + (size_t)(w * F / V) * row;
    for (size_t k = 0; k < row; ++k) centres_out[(size_t)w * row + k] = src[k];
  }
  if (int rc = select_device(device)) return rc;
  std::vector<uint32_t> count(nv);
  Staged S;
  const int h_desc = S.in(desc, nf * row);
  const int h_cen = S.out(centres_out, nv * row), h_count = S.out(count.data(), nv * sizeof(uint32_t));
  const int h_nrm = S.out(nullptr, nf * sizeof(int32_t), true), h_cnrm = S.out(nullptr, nv * sizeof(int32_t), true);
  const int h_wa = S.out(nullptr, nf * sizeof(int32_t), true), h_wb = S.out(nullptr, nf * sizeof(int32_t), true);
  const int h_wd = S.out(nullptr, nf * sizeof(int32_t), true), h_sums = S.out(nullptr, nv * row * sizeof(uint32_t), true);
  const int h_scal = S.out(nullptr, 2 * sizeof(unsigned long long), true);
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  uint8_t *cen = S.ptr<uint8_t>(h_cen);
  if (hipMemcpy(cen, centres_out, nv * row, hipMemcpyHostToDevice) != hipSuccess) return FGO_ENUM;
  const uint8_t *d_desc = S.ptr<uint8_t>(h_desc);
  int32_t *nrm = S.ptr<int32_t>(h_nrm), *cnrm = S.ptr<int32_t>(h_cnrm), *cur = S.ptr<int32_t>(h_wa), *prev = S.ptr<int32_t>(h_wb);
  int32_t *wd = S.ptr<int32_t>(h_wd);
  uint32_t *d_count = S.ptr<uint32_t>(h_count), *sums = S.ptr<uint32_t>(h_sums);
  unsigned long long *scal = S.ptr<unsigned long long>(h_scal), host_scal[2] = {0, 0};
  const unsigned g_stats = grid_for((unsigned long long)F, 256 * 16), g_sums = grid_for((unsigned long long)F * row, 256 * 8);

  // assign with the centres as they are, then the counts, the changed-count against `against` (NULL: none) and the inertia
  auto assign = [&](bool first, const int32_t *against) -> bool {
    launch_assign(F, d_desc, nrm, first, V, cen, cnrm, cur, wd);
    (void)hipMemsetAsync(d_count, 0, nv * sizeof(uint32_t), 0);
    (void)hipMemsetAsync(scal, 0, sizeof(host_scal), 0);
    hipLaunchKernelGGL(k_place_stats, dim3(g_stats), dim3(256), 0, 0, F, cur, against, wd, d_count, scal);
    return hipMemcpy(host_scal, scal, sizeof(host_scal), hipMemcpyDeviceToHost) == hipSuccess;
  };
  fgo_vocab_result R = {0, 0, -1, 0, 0};
  KernelTimer timer;
  if (!timer.start()) return FGO_ENUM;
  for (int it = 0; it < P.n_iters; ++it) {
    if (!assign(it == 0, it == 0 ? nullptr : prev)) return FGO_ENUM;
    R.changed_last = it == 0 ? F : (int64_t)host_scal[0];
    if (R.changed_last == 0) { R.converged = 1; break; }
    (void)hipMemsetAsync(sums, 0, nv * row * sizeof(uint32_t), 0);
    hipLaunchKernelGGL(k_place_sums, dim3(g_sums), dim3(256), 0, 0, F, d_desc, cur, sums);
    hipLaunchKernelGGL(k_place_update, dim3((unsigned)((nv * row + 255) / 256)), dim3(256), 0, 0, V, sums, d_count, cen);
    int32_t *t = cur; cur = prev; prev = t;
    ++R.iterations;
  }
  // a converged loop's last assign was made with the final centres: its counts and inertia are the result
  if (!R.converged && !assign(P.n_iters == 0, nullptr)) return FGO_ENUM;
  timer.stop();
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  g_place_kernel_ms = timer.ms();
  if (int rc = S.download()) return rc;
  R.inertia = (int64_t)host_scal[1];
  for (size_t w = 0; w < nv; ++w) {
    count_out[w] = count[w];
    R.n_empty += count[w] == 0;
  }
  *result = R;
  return FGO_OK;
}

extern "C" int fgo_place_query_batch(int device, int64_t n_frames, const int64_t *feat_ptr, const uint8_t *desc, int V, const uint8_t *centres,
                                     const int32_t *weight_in, const fgo_place_params *params, int32_t *word_out, int32_t *word_d_out,
                                     int32_t *df_out, int32_t *weight_out, int64_t *norm2_out, int32_t *n_cand_out, int64_t *cand_frame_out,
                                     int64_t *cand_dot_out, double *cand_score_out, int64_t *pair_i_out, int64_t *pair_j_out,
                                     int64_t *n_pairs_out, int64_t *dot_out) {
  using namespace fgo;
  fgo_place_params P;
  fgo_place_params_default(&P);
  if (params) P = *params;
  if (n_frames < 0 || n_frames > INT_MAX || !vocab_size_ok(V)) return FGO_EINVAL;
  if (P.top_k < 1 || P.top_k > PL_K || P.min_gap < 1 || !in_closed(P.min_score, 0.0, 1.0)) return FGO_EINVAL;
  if (P.max_df_permille < 0 || P.max_df_permille > 1000 || !pair_i_out != !pair_j_out) return FGO_EINVAL;
  if (n_frames == 0) {
    if (n_pairs_out) *n_pairs_out = 0;
    return FGO_OK;
  }
  if (!feat_ptr || !desc || !centres || !cand_frame_out || !cand_dot_out || !cand_score_out) return FGO_EINVAL;
  if (!csr_ptr_ok(feat_ptr, n_frames, FGO_FM_MAX_FEATURES)) return FGO_EINVAL;
  if (weight_in)
    for (int w = 0; w < V; ++w)
      if (weight_in[w] < 0 || weight_in[w] > 65535) return FGO_EINVAL;
  const size_t N = (size_t)n_frames, nv = (size_t)V, K = (size_t)P.top_k;
  const int64_t F = feat_ptr[n_frames];                      // the arrays are indexed by feat_ptr's own values
  const size_t nf = (size_t)F, I4 = sizeof(int32_t), I8 = sizeof(int64_t);
  if (int rc = select_device(device)) return rc;

  std::vector<int32_t> df_own, q_own;
  if (!df_out) { df_own.resize(nv); df_out = df_own.data(); }
  if (!weight_out) { q_own.resize(nv); weight_out = q_own.data(); }
  Staged S;
  const int h_fp = S.in(feat_ptr, (N + 1) * I8), h_desc = S.in(desc, nf * FGO_FM_DIM), h_cen = S.in(centres, nv * FGO_FM_DIM);
  const int h_nrm = S.out(nullptr, nf * I4, true), h_cnrm = S.out(nullptr, nv * I4, true);
  const int h_word = S.out(word_out, nf * I4, true), h_wd = S.out(word_d_out, nf * I4, true);
  const int h_lw = S.out(nullptr, nf * I4, true), h_lv = S.out(nullptr, nf * I4, true), h_ln = S.out(nullptr, N * I4, true);
  const int h_df = S.out(nullptr, nv * I4, true), h_q = S.out(nullptr, nv * I4, true);       // copied by hand, between the launches
  const int h_n2 = S.out(norm2_out, N * I8, true), h_nc = S.out(n_cand_out, N * I4);
  const int h_cf = S.out(cand_frame_out, N * K * I8), h_cd = S.out(cand_dot_out, N * K * I8), h_cs = S.out(cand_score_out, N * K * sizeof(double));
  const int h_dot = S.out(dot_out, N * N * I8);
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  const int64_t *d_fp = S.ptr<int64_t>(h_fp);
  int32_t *word = S.ptr<int32_t>(h_word), *lw = S.ptr<int32_t>(h_lw), *lv = S.ptr<int32_t>(h_lv), *ln = S.ptr<int32_t>(h_ln);
  int32_t *d_df = S.ptr<int32_t>(h_df), *d_q = S.ptr<int32_t>(h_q);
  const size_t lds = std::max(nv * I4, (size_t)PL_MERGE_BYTES);
  if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_place_score), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return FGO_ENUM;

  KernelTimer t_assign, t_hist, t_score;
  if (!t_assign.start()) return FGO_ENUM;
  launch_assign(F, S.ptr<uint8_t>(h_desc), S.ptr<int32_t>(h_nrm), true, V, S.ptr<uint8_t>(h_cen), S.ptr<int32_t>(h_cnrm), word,
                S.ptr<int32_t>(h_wd));
  t_assign.stop();
  if (!t_hist.start()) return FGO_ENUM;
  (void)hipMemsetAsync(d_df, 0, nv * I4, 0);
  hipLaunchKernelGGL(k_place_hist, dim3(grid_for(N, 1)), dim3(PL_T), 0, 0, n_frames, d_fp, word, V, lw, lv, ln, d_df);
  t_hist.stop();
  if (hipMemcpy(df_out, d_df, nv * I4, hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;

  // ---- the weights, on the host: the caller's, or the inverse document frequency in 1 / 256 bits
  for (size_t w = 0; w < nv; ++w) {
    const int64_t d = df_out[w];
    if (weight_in) weight_out[w] = weight_in[w];
    else if (d == 0 || 1000 * d > (int64_t)P.max_df_permille * n_frames) weight_out[w] = 0;
    else weight_out[w] = (int32_t)std::floor(256.0 * std::log2((double)n_frames / (double)d));
  }
  if (hipMemcpy(d_q, weight_out, nv * I4, hipMemcpyHostToDevice) != hipSuccess) return FGO_ENUM;

  ScoreArgs A;
  A.n_frames = n_frames; A.feat_ptr = d_fp; A.norm2 = S.ptr<int64_t>(h_n2); A.ln = ln; A.lw = lw; A.lv = lv;
  A.V = V; A.top_k = P.top_k; A.min_gap = P.min_gap; A.min_score = P.min_score;
  A.n_cand = S.ptr<int32_t>(h_nc); A.cand_frame = S.ptr<int64_t>(h_cf); A.cand_dot = S.ptr<int64_t>(h_cd); A.dot = S.ptr<int64_t>(h_dot);
  A.cand_score = S.ptr<double>(h_cs);
  if (!t_score.start()) return FGO_ENUM;
  hipLaunchKernelGGL(k_place_weigh, dim3(grid_for(N, 4)), dim3(256), 0, 0, n_frames, d_fp, ln, lw, lv, d_q, S.ptr<int64_t>(h_n2));
  hipLaunchKernelGGL(k_place_score, dim3(grid_for(N, 1)), dim3(PL_T), lds, 0, A);
  t_score.stop();
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  g_place_phase_ms[0] = t_assign.ms(); g_place_phase_ms[1] = t_hist.ms(); g_place_phase_ms[2] = t_score.ms();
  g_place_kernel_ms = g_place_phase_ms[0] + g_place_phase_ms[1] + g_place_phase_ms[2];
  if (int rc = S.download()) return rc;

  // ---- the host packs: ascending j, then rank
  if (pair_i_out) {
    int64_t m = 0;
    for (size_t a = 0; a < N; ++a)
      for (size_t r = 0; r < K && cand_frame_out[a * K + r] >= 0; ++r) {
        pair_i_out[m] = cand_frame_out[a * K + r];
        pair_j_out[m] = (int64_t)a;
        ++m;
      }
    if (n_pairs_out) *n_pairs_out = m;
  }
  return FGO_OK;
}
