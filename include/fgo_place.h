/*
 * fgo_place.h — place recognition by visual words on the device: which OLD key frames to try against a key frame.
 *
 * Everything in fgo.h from fgo_match_features_batch on takes frame_i / frame_j as input; the reference only ever pairs a key frame
 * with the last m_lookback_nodes ones (g2o/g2o_graph.cpp:195-205, gtsam/gt_parameter.cpp:15), so a revisit after a long excursion
 * never becomes an edge.  The two calls below turn descriptors into a short list of old key frames per key frame, in the form
 * fgo_match_features_batch takes.  A bag-of-words retrieval is not part of the reference tree (the VRO library is not vendored):
 * the semantics below are THIS PROJECT'S DEFINITION, pinned to the numpy restatement tests/place_reference.py, itself pinned to
 * brute force by tests/test_place_reference_cpu.py.
 *
 * Common to both calls
 *   descriptors  F x 128 bytes (FGO_FM_DIM), integers 0 .. 255.  d(a, b) = sum_k (a[k] - b[k])^2, an integer <= 128 * 255^2 =
 *                8 323 200, computed exactly.
 *   validity     every feature counts: there is no depth test here.
 *   order        frames are in key-frame order: the index is time.
 *   assign       a feature goes to the centre (word) w with the least d; ties go to the lowest w.
 * Both calls are stateless, host arrays in and out, like fgo_match_features_batch; FGO_ENODEV without a HIP device (no CPU
 * fallback).  The arithmetic is integer up to the score, the sums are integer atomics whose result does not depend on their order:
 * two calls are bit-identical.
 */
#ifndef FGO_PLACE_H
#define FGO_PLACE_H
#include "fgo.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FGO_PLACE_MAX_WORDS 16384
#define FGO_PLACE_MAX_TRAIN 16777216   /* 2^24 descriptors in one fgo_vocab_train: 255 * 2^24 < 2^32, a byte sum fits 32 bits */

/* A vocabulary of V = n_words centres by deterministic integer Lloyd iterations over desc (F x 128).
 *   init      centre w is descriptor floor(w * F / V), the product in int64.
 *   loop      for it in 0 .. n_iters - 1: assign; changed = F when it == 0, otherwise the number of features whose word is not the
 *             one of the assignment before; changed == 0 stops the loop with converged = 1; otherwise update.
 *   update    a word with n > 0 members: every byte becomes floor((2 * sum + n) / (2 * n)) over its members' bytes (round half up,
 *             in integers).  A word with no member keeps its centre.
 *   result    after the loop one more assign gives count_out (the members of every word), inertia = the sum of d over the features
 *             and n_empty = the words without a member.  iterations = the updates done; changed_last = the `changed` of the last
 *             assign of the loop, -1 when n_iters == 0 (the loop made none).
 * The sums are integer atomics: two calls are bit-identical, and permuting descriptors that do not move the initial picks changes
 * nothing.  FGO_EINVAL (before any HIP call): a NULL desc, centres_out, count_out or result, n_words < 1 or > FGO_PLACE_MAX_WORDS,
 * F < n_words, F > FGO_PLACE_MAX_TRAIN, n_iters < 0. */
typedef struct {
  int n_words;   /* 1024 */
  int n_iters;   /* 10 */
} fgo_vocab_params;
void fgo_vocab_params_default(fgo_vocab_params *p);        /* NULL tolerated */
typedef struct {
  int iterations;
  int converged;
  int64_t changed_last;
  int64_t inertia;
  int64_t n_empty;
} fgo_vocab_result;
int fgo_vocab_train(int device, int64_t F, const uint8_t *desc /* F x 128 */, const fgo_vocab_params *params /* NULL = defaults */,
                    uint8_t *centres_out /* V x 128 */, int64_t *count_out /* V */, fgo_vocab_result *result);

/* The candidates of every key frame: words, weights, scores, top-k.  Frame n owns the features [feat_ptr[n], feat_ptr[n+1]) of
 * desc; centres (V x 128) is a vocabulary, fgo_vocab_train's or any other.
 *   words       word[f] = the assignment above, word_d[f] its distance.  c[n][w] = the features of frame n with word w, df[w] = the
 *               frames with c[n][w] > 0.
 *   weights     q[w] = weight_in[w] when weight_in is given (0 <= weight_in[w] <= 65535).  Otherwise q[w] = 0 if df[w] == 0 or
 *               1000 * df[w] > max_df_permille * N (a stop word; N = n_frames, the products in int64), and otherwise
 *               q[w] = (int32) floor(256.0 * log2((double) N / (double) df[w])), formed ON THE HOST in f64 with the C library's
 *               log2: it is exact where N / df is a power of two and may differ by one from another libm elsewhere.  The table
 *               used is always what weight_out returns; pass it back as weight_in to score other frames with the same weights.
 *   vectors     v[n][w] = c[n][w] * q[w];  norm2[n] = sum_w v[n][w]^2;  dot(a, b) = sum_w v[a][w] v[b][w].  Both in int64, exact:
 *               c <= FGO_FM_MAX_FEATURES = 4096 and q <= 65535 give v < 2^31, and the counts of a frame sum to at most 4096, so
 *               both sums stay at or below (4096 * 65535)^2 < 2^63.
 *   score       s(a, b) = (double) dot / sqrt((double) norm2[a] * (double) norm2[b]): one multiply, one square root and one divide,
 *               each correctly rounded, nothing contracted; s = 0 when either norm is 0.
 *   database    of frame a: the frames b <= a - min_gap, min_gap >= 1 (the look-back handles the nearer ones).  Every unordered
 *               pair is scored once.
 *   candidates  of frame a: the first top_k, in the order (s descending, b ascending), of the database frames with dot > 0 and
 *               s >= min_score.
 * Outputs.  Per feature: word_out, word_d_out.  Per word: df_out, weight_out.  Per frame: norm2_out, n_cand_out (the candidates
 * found, <= top_k).  Candidates, with the stride top_k per frame, rank after rank: cand_frame_out (padded with -1), cand_dot_out
 * (padded with 0), cand_score_out (padded with 0).  Pair lists, packed by the host after the download, capacity N * top_k, the first
 * *n_pairs_out filled, ordered by ascending j and then by rank: pair_i_out (the old frame b) and pair_j_out (the new frame a) --
 * exactly what fgo_match_features_batch takes as frame_i, frame_j (both or neither; *n_pairs_out is written with them).  dot_out (for tests and diagnosis, like dist_out): N x N int64,
 * row a, column b, -1 outside the database of a; without it the device memory of a call does not grow as N^2.
 * A frame's words and norm do not depend on the rest of the batch when weight_in is given.
 * FGO_EINVAL (before any HIP call): a NULL feat_ptr, desc, centres, cand_frame_out, cand_dot_out or cand_score_out; exactly one of
 * pair_i_out and pair_j_out; a negative n_frames; a negative or decreasing feat_ptr; more than FGO_FM_MAX_FEATURES features in a
 * frame; V < 1 or > FGO_PLACE_MAX_WORDS; top_k outside [1, 64]; min_gap < 1; min_score outside [0, 1] or NaN; max_df_permille
 * outside [0, 1000]; a weight_in outside [0, 65535].  n_frames == 0: FGO_OK, *n_pairs_out = 0. */
typedef struct {
  int top_k;             /* 5 */
  int min_gap;           /* 10: the reference's look-back (m_lookback_nodes, 5 to 10 in its launch files) covers the nearer frames */
  double min_score;      /* 0.0 */
  int max_df_permille;   /* 1000: no stop words */
} fgo_place_params;
void fgo_place_params_default(fgo_place_params *p);        /* NULL tolerated */
int fgo_place_query_batch(int device, int64_t n_frames, const int64_t *feat_ptr /* n_frames + 1 */, const uint8_t *desc /* F x 128 */,
                          int V, const uint8_t *centres /* V x 128 */, const int32_t *weight_in /* V, or NULL */,
                          const fgo_place_params *params /* NULL = defaults */,
                          int32_t *word_out /* F, may be NULL */, int32_t *word_d_out /* F, may be NULL */,
                          int32_t *df_out /* V, may be NULL */, int32_t *weight_out /* V, may be NULL */,
                          int64_t *norm2_out /* N, may be NULL */, int32_t *n_cand_out /* N, may be NULL */,
                          int64_t *cand_frame_out /* N x top_k */, int64_t *cand_dot_out /* N x top_k */,
                          double *cand_score_out /* N x top_k */,
                          int64_t *pair_i_out /* N x top_k, may be NULL */, int64_t *pair_j_out /* N x top_k, may be NULL */,
                          int64_t *n_pairs_out /* 1, may be NULL */, int64_t *dot_out /* N x N, may be NULL: for tests and diagnosis */);
/* development: the kernel time of the last fgo_place_query_batch or fgo_vocab_train call by HIP events, ms; and of the last
 * fgo_place_query_batch its parts: out[0] the assign kernel (with the norms), out[1] the histogram, out[2] the scoring */
double fgo_debug_place_kernel_ms(void);
void fgo_debug_place_phase_ms(double out[3]);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FGO_PLACE_H */
