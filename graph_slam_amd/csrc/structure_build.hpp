// Structure phase of libfgo, internal to its translation units (fgo_structure.cpp and structure_*.cpp): what each phase of
// build() produces for the later ones, and the encodings that build() and the in-place growth (refresh_factors) share.
#pragma once
#include "fgo_ctx.hpp"
#include <thread>

namespace fgo {

// ---- phase outputs.  A phase takes what it reads by const reference and fills its own struct; build_phases (fgo_structure.cpp)
// holds them and releases them on a detached thread.
struct VarIndex {                        // classify
  int64_t N = 0, E = 0, NI = 0;          // variables, binary factors, IMU factors of the context
  int64_t R = 0, NX = 0;                 // phantom variables of the growth reserve, N + R
  int isam_window = 0;
  std::vector<int> lm_index;             // [NX] number of an eliminated landmark (-1: a column of the block system)
  int n_lm = 0;
  std::vector<int> hidx;                 // [NX] free-variable (hessian) index, -1: fixed or eliminated
  int nfree = 0;
};
struct PairRec { int a, b; int64_t e; };                                          // hessian indices a < b; e: edge, -1 - (15 f + q) IMU pair
constexpr int64_t STRUCT_ONLY = std::numeric_limits<int64_t>::min();              // PairRec::e of a pair without a factor (yet)
struct PairGraph {                       // pairs_and_graph
  std::vector<PairRec> pr;               // sorted by (a, b, e)
  std::vector<int> ua, ub;               // unique pairs
  std::vector<int64_t> ufirst;           // [noff + 1] index in pr of a pair's first member
  int64_t noff = 0;
  BlockGraph g;
  std::vector<int> adj_pair;             // pair index of every adjacency entry of g
};
struct Ordering {                        // order_and_symbolic (the symbolic factorisation itself is fgo_ctx::S)
  std::vector<int> perm;
  int world = 0, rank = 0, nb = 0;
  bool dist = false;
  int top_col0 = 0;
  int64_t top_blk0 = 0;
  double t_ord = 0;                      // seconds in nested_dissection
};
struct HostTables {                      // host_tables
  std::vector<int> pose_col, asrc, ptri_src, prow_src;
  std::vector<int> edge_slot, dup_slot, imu_slot, imu_list;
  std::vector<int64_t> dup_ptr, dup_edges;
  std::vector<int64_t> he_ptr, imu_inc_ptr;
  std::vector<int> he, imu_inc;
  std::vector<unsigned char> var_mine;
  std::vector<int64_t> top_ext0, own_op0, own_op1, top_row0, own_row0, own_row1;   // distributed offsets
  std::vector<double, NoInitAlloc<double>> erec;
  int64_t E_cap = 0, NI_cap = 0;
};
struct BaTables {                        // landmark elimination (structure_ba.cpp; device_plan.hpp "BaPlan")
  std::vector<unsigned char> lm_mine;    // distributed: [n_lm] this rank eliminates the landmark (empty: all)
  std::vector<int> lm_var, pt_obs, obs_edge, obs_cam, obs_col, obs_lm, cam_col, tgt_blk, op_a, op_b, op_lm, tgt_list, cam_list;
  std::vector<int64_t> pt_ptr, cam_ptr, tgt_ptr, cam_t0;
  std::vector<double> obs_uvw;
  int n_small = 0;
  int64_t o_first = 0;
};
struct BuildTimer {                      // FGO_SYM_PROFILE: one line per phase
  bool prof = false;
  double tprev = 0;
  void lap(const char *what) { if (prof) { const double t = now_s(); std::fprintf(stderr, "[fgo build]    %-28s %.1f ms\n", what, 1e3 * (t - tprev)); tprev = t; } }
};

// ---- phases (build_phases calls them in this order)
int pairs_and_graph(fgo_ctx *c, const VarIndex &V, PairGraph &G, BuildTimer &tm);                                  // structure_pairs.cpp
int host_tables(fgo_ctx *c, const VarIndex &V, const PairGraph &G, const Ordering &O, HostTables &T,
                std::vector<unsigned char> &lm_mine, BuildTimer &tm);                                              // structure_tables.cpp
int upload_structure(fgo_ctx *c, const VarIndex &V, const PairGraph &G, const Ordering &O, const HostTables &T,
                     const BaTables &BA, BuildTimer &tm);                                                          // structure_upload.cpp
// structure_ba.cpp: the landmark-elimination part of every phase
void ba_select_landmarks(const fgo_ctx *c, VarIndex &V);
void ba_covisibility_pairs(const fgo_ctx *c, const VarIndex &V, std::vector<PairRec> &pr);
int ba_landmark_owners(fgo_ctx *c, const VarIndex &V, const Ordering &O, std::vector<unsigned char> &lm_mine);
int ba_tables(fgo_ctx *c, const VarIndex &V, const PairGraph &G, const Ordering &O, const HostTables &T, BaTables &BA, BuildTimer &tm);
int ba_upload(fgo_ctx *c, const VarIndex &V, const Ordering &O, const BaTables &BA);

// delete p on a detached thread: unmapping a few hundred MB of host tables takes tens of milliseconds.  (Must not throw: when no
// thread can be created -- EAGAIN under a pids / ulimit cap -- the tables are released here, on the caller's time.)
template <class T>
void release_detached(T *p) noexcept { try { std::thread([p] { delete p; }).detach(); } catch (...) { delete p; } }

// ---- encodings shared by the build and the in-place growth
// H slot of a factor's off-diagonal block: H block nb + pair, bit 0 set when the block is stored transposed (the second variable
// is eliminated later than the first)
inline int h_slot(int64_t nb, int64_t pair, int col_i, int col_j) { return (int)(((nb + pair) << 1) | (col_j > col_i ? 1 : 0)); }
// two hessian indices couple through an off-diagonal block (a fixed or eliminated end needs none)
inline bool needs_pair(int a, int b) { return a >= 0 && b >= 0 && a != b; }
inline uint64_t pair_key(int a, int b) { return ((uint64_t)(uint32_t)std::min(a, b) << 32) | (uint32_t)std::max(a, b); }
// variable pair (u < w) number q of a 6-variable IMU factor
constexpr unsigned char IMU_PAIR[15][2] = {{0, 1}, {0, 2}, {0, 3}, {0, 4}, {0, 5}, {1, 2}, {1, 3}, {1, 4}, {1, 5}, {2, 3}, {2, 4}, {2, 5}, {3, 4}, {3, 5}, {4, 5}};
// payload of edge e: inverse measurement for the SE3 kinds (raw otherwise), then the 21 information entries
inline void edge_payload(const fgo_ctx *c, int64_t e, double *meas7, double *info21) {
  if (c->torder[e] <= 1) pose_inv7(&c->meas[(size_t)e * 7], meas7);
  else std::memcpy(meas7, &c->meas[(size_t)e * 7], 7 * sizeof(double));
  std::memcpy(info21, &c->info[(size_t)e * 21], 21 * sizeof(double));
}

// ---- structure_grow.cpp: what both sides call
// Linearisation hubs (device_plan.hpp): the degree limit of this graph, one entry per slice of every hub variable, and the
// list of the hubs that have several slices.  deg_limit == 0: choose it.
struct HubPlan {
  int deg_limit = HUB_DEG;
  std::vector<int> var, slice;          // per entry
  std::vector<int> multi;               // 3 per multi-slice hub: variable, first entry, slices
};
// entries (slices) of a variable of degree d: 0 up to the graph's degree limit
inline int hub_slices(int64_t d, int deg_limit) { return d > deg_limit ? (int)std::min<int64_t>(HUB_MAX_SLICES, (d + HUB_SLICE - 1) / HUB_SLICE) : 0; }
void plan_hubs(const std::vector<int64_t> &he_ptr, int64_t NX, int deg_limit, HubPlan &hp);
int upload_hubs(fgo_ctx *c, const HubPlan &hp, size_t entry_cap);
int upload_priors(fgo_ctx *c, int64_t NX, const std::vector<unsigned char> &mine);
void imu_colour_add(fgo_ctx *c, int64_t f);
void imu_colour_lists(fgo_ctx *c, std::vector<int> &sorted);
void set_factor_plan(fgo_ctx *c, int64_t N, int64_t E, int64_t NI, const HubPlan &hubs, int64_t n_dup_groups);
void snapshot_for_growth(fgo_ctx *c, const VarIndex &V, const PairGraph &G, const Ordering &O, const HostTables &T, int hub_deg, size_t hub_cap);

}  // namespace fgo
