// Shared declarations of the tabular-solver translation units (round 6: osg_cfr.hip split by kernel family):
//
//   osg_cfr.hip         the flattened tree (build_tree), the tables, the C-ABI entry points and their dispatch
//   osg_cfr_small.hip   k_cfr, k_cfr_small            one workgroup (kuhn_poker; any small tree)
//   osg_cfr_split.hip   k_cfr_split                   one workgroup per deal subtree (leduc_poker)
//   osg_cfr_sub.hip     k_cfr_sub, k_gcfr_*           one persistent cooperative launch / a launch per phase (3-player leduc)
//   osg_cfr_eval.hip    k_policy_eval, k_geval_*, k_eval_jobs     ExpectedReturns / TabularBestResponse / NashConv
//   osg_cfr_qvalues.hip k_qvalues_small, k_qv_*       per-infostate action values and reaches of a policy
//   osg_cfr_mccfr.hip   k_mccfr*, k_os_mccfr*, ...    external / outcome sampling MCCFR and their entry points
//   osg_cfr_population.hip k_pop_*                    payoff-tensor cells and policy aggregation of a population of tables
//
//   osg_cfr_xfp.hip     k_xfp_small, k_xfp_*          extensive-form fictitious play
//   osg_cfr_mmd.hip     k_mmd_small, k_mmd_*          magnetic mirror descent (MmdState lives there)
//   osg_cfr_efr.hip     k_efr_resident, k_efr_*       extensive-form regret minimization (osg_efr.h has the arithmetic)
//   osg_deep_cfr.hip    k_dcfr_*, k_res_*             Deep CFR traversals and reservoir buffers (osg_deep_cfr.h has the arithmetic)
//   osg_nfsp.hip        k_nfsp_*, k_ring_*            NFSP self-play episodes and the DQN transition ring (osg_nfsp.h has the arithmetic)
//
// Every kernel is launched from the translation unit that defines it; what crosses the units are the device-side
// argument structs below (views: raw pointers), the per-family plans that own the memory behind them (SplitPlan,
// SubPlan, EvalPlan, JobsPlan, ResidentPlan: DeviceArray / PinnedArray of osg_device_buffer.h), struct osg_cfr, the one
// function per family that forms a view from its plan, and the host functions declared at the end.
//
// What a plan holds is worked out by the host-only planners of osg_cfr_plan.h (no HIP, no environment: they compile and
// are tested without a device) from osg_cfr::host_tree(): plan_split feeds k_cfr_split, plan_sub and plan_sub_fold
// k_cfr_sub, plan_eval_jobs k_eval_jobs, plan_resident the k_mccfr_resident* / k_os_mccfr_resident kernels, and
// mccfr_launch_plan picks the MCCFR kernel and geometry of a mini-batch.  The build_* functions add what needs the device
// (LDS caps, occupancy, uploads); the node kinds and the kernels' size limits the planners share live in that header too.
// Reference files: cfr.{h,cc},
// external_sampling_mccfr.{h,cc}, outcome_sampling_mccfr.cc, cfr_br.cc, expected_returns.cc, best_response.cc.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "osg_cfr_plan.h"
#include "osg_efr.h"
#include "osg_internal.h"

using namespace osg;

namespace osg_cfr_impl {

constexpr int kMaxPolicyRow = 8;  // widest policy row a thread regret-matches in registers (kuhn 2, leduc 3)
constexpr double kMccfrInit = 0.000001;  // external_sampling_mccfr.h:59 kInitialTableValues

// The launch forms the choosers below struct osg_cfr pick.  Policy evaluation: k_policy_eval, k_eval_jobs, k_geval_*;
// kGridPersist is never chosen: recorded where kGrid took its opt-in persistent launch (OSG_EVAL_PERSIST=1).
enum class EvalForm { kOneWorkgroup, kJobs, kGrid, kGridPersist };
enum class CfrForm { kSub, kGrid, kSplit, kSmall };   // k_cfr_sub, k_gcfr_*, k_cfr_split, one workgroup (k_cfr_small / k_cfr)

struct Tree {  // device pointers
  int H, I, A, P, D;
  const int32_t* level_off;    // [D+1]
  const int32_t* parent;       // [H]
  const int32_t* first_child;  // [H]
  const uint8_t* kind;         // [H]
  const uint8_t* nchild;       // [H]
  const uint8_t* aidx;         // [H] index of the incoming edge among the parent's children
  const int8_t* actor;         // [H] acting player, -1 at chance / terminal nodes
  const int32_t* info;         // [H] infostate id of a decision node, else -1
  const double* edge_prob;     // [H] chance probability of the incoming edge (parent is chance)
  const double* term_ret;      // [H, P] Returns() of terminal nodes
  const int32_t* mem_off;      // [I+1]
  const int32_t* mem;          // member histories of every infostate, DFS order
  const int32_t* nact;         // [I]
  const int8_t* info_player;   // [I]
};

struct Tables {  // [I, A] fp64
  double* regrets;
  double* cum;
  double* cur;
};

// ---------------------------------------------------------------------------
// CFRInfoStateValues::ApplyRegretMatching (cfr.cc:596-615) on one row.
// ---------------------------------------------------------------------------
OSG_D void regret_match_row(const double* regrets, double* policy, int n) {
  double sum_pos = 0.0;
  for (int a = 0; a < n; ++a)
    if (regrets[a] > 0) sum_pos += regrets[a];
  for (int a = 0; a < n; ++a) {
    if (sum_pos > 0) policy[a] = regrets[a] > 0 ? regrets[a] / sum_pos : 0.0;
    else policy[a] = 1.0 / n;
  }
}

// ---------------------------------------------------------------------------
// Discounted CFR (discounted_cfr.py:190-209): the factors of one iteration t — t^alpha / (t^alpha + 1) for a regret
// that is >= 0 after the pass's terms were added, t^beta / (t^beta + 1) for a negative one, and the averaging weight
// t^gamma.  They are formed on the host (discount_factors: std::pow in double precision, what the reference's `**`
// calls) and reach a launch as a table of three doubles per iteration of that launch: the index is the launch's loop
// counter, so the three loads are wave-uniform.  The kernels take discounting as a template parameter (kDcfr): the
// plain CFR / CFR+ instantiations hold none of it.
// ---------------------------------------------------------------------------
struct Discount { double pos, neg, weight; };
OSG_D Discount discount_of(const double* __restrict__ table, int it) {
  Discount f{table[3 * it], table[3 * it + 1], table[3 * it + 2]};
  // (fetched by scalar loads, then kept in vector registers: six more scalar registers held across an iteration were
  // parked in vector lanes by kernels that already sit at the scalar file's limit)
  asm volatile("" : "+v"(f.pos), "+v"(f.neg), "+v"(f.weight));
  return f;
}
OSG_D double discounted(double regret, const Discount& f) { return regret * (regret >= 0 ? f.pos : f.neg); }

struct SmallTree {  // device pointers to the extra host-built arrays
  const int32_t* path_off;    // [M+1] per decision history (member order)
  const int32_t* path;        // entries: slot << 24 | is_chance << 23 | index
  int M;                      // decision histories
  int n_path;
  int L0 = 0;                 // the first level that holds a decision history: the sweep of k_cfr_small stops there — the
                              // values of the chance levels above (the deals) are read by nobody (phase B reads a decision
                              // history's own value and its children's), and for kuhn_poker they were 2 of its 5 level steps
};

struct SmallGlobal {  // global-memory homes of the same arrays, for trees too big for LDS (leduc)
  double* value;         // [H, P]
  double* dreg;          // [M, A]
  double* dpol;          // [M, A]
  int32_t* skip;         // [M]
  const int32_t* meta;   // [H] kind | nchild << 2 | (actor + 1) << 10
  const int32_t* info_player;  // [I]
};

struct SplitTree {
  int G, L, NL, NM, NI;          // subtrees, cut level, padded histories / members / infostates per subtree
  const int32_t* nloc;           // [G] histories of the subtree
  const int32_t* hist_desc;      // [G, NL] kind | nchild << 2 | level << 10 | (actor + 1) << 16
  const int32_t* hist_fc;        // [G, NL] LOCAL index of the first child
  const int32_t* hist_row;       // [G, NL] info * A of a decision node
  const int32_t* hist_glob;      // [G, NL] the history's index in the whole tree
  const int32_t* mem_m;          // [G, NM] member index (position in Tree::mem), -1 = padding
  const int32_t* mem_hloc;       // [G, NM] its history, local index
  const int32_t* info_list;      // [G, NI] infostates with a member in the subtree, -1 = padding
  double* terms;                 // [2][M][kSplitRec]: buffer (pass parity) x {own reach or -1, A regret terms} per member
  unsigned int* bar;             // [0] arrival counter (zero between launches), [1] error flag, [2] sticky error, [3] exit counter
  unsigned int* host_err;        // pinned host word raised on a timeout: the host's next call reads it without a copy
};

OSG_D void store_through(double* p, double v) {   // agent scope: written through to memory, visible to every CU
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(__double_as_longlong(v)),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
OSG_D double load_through(const double* p) {      // agent scope: never served from a stale L1 / L2 line
  return __longlong_as_double(static_cast<long long>(__hip_atomic_load(
      reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
}

constexpr int kSplitRec = 1 + kSplitMaxA;  // doubles per member and buffer: own reach, regret terms
constexpr int kSplitChunk = 6;       // members whose records are requested together

struct GridCfr {
  Tree t;
  const int32_t* path_off;
  const int32_t* path;
  const int32_t* meta;         // [H] kind | nchild << 2 | (actor + 1) << 10
  const int32_t* info_player;  // [I]
  double* value;               // [H, P]
  double* dreg;                // [M, A]
  double* dpol;                // [M, A]
  int32_t* skip;               // [M]
  Tables tb;
  int M;
  const double* pol = nullptr; // [I, A] the policy a pass plays: tb.cur, or CFR-BR's effective policy (k_gcfr_effpol)
};

struct SubTree {
  int G, L, NL;                  // subtrees, cut level, padded histories per subtree
  const int32_t* nloc;           // [G] histories of the subtree
  const int32_t* desc;           // [G, NL] kind | nchild << 2 | level << 10 | (actor + 1) << 16
  const int32_t* fc;             // [G, NL] LOCAL index of the first child
  const int32_t* aux;            // [G, NL] decision: its index d among the subtree's decision histories; chance /
                                 //          terminal: the history's global index
  int ND;                        // padded decision histories per subtree
  const int32_t* ndec;           // [G]
  const int32_t* dec_row;        // [G, ND] info * A of decision history d
  const int32_t* mem_off;        // [G * P + 1] the subtree's members of player q: sub_mem[mem_off[g * P + q] ...)
  const int32_t* sub_rec;        // [., 8 + PL / 2 rounded up to 4] (the codes are 16-bit halves, 0xFFFF padded) per member: m (position in Tree::mem), its history's local index, its decision
                                 //   index | actions << 24, its first child's local index; the product of the chance
                                 //   probabilities on its root path (a double, path order), two unused words; then the decision
                                 //   entries of the path GROUPED BY PLAYER, PL / P codes per player in path order, -1 padded:
                                 //   (the ancestor's decision index in this subtree) * A + action index, i.e. an index into the
                                 //   policy rows the sweep has staged in LDS
  int PL;                        // codes per member: P groups of a multiple of 4, at most 4 kSubCodeChunks
  const int32_t* info_off;       // [P + 1] infostates of player q: info_list[info_off[q] ...)
  const int32_t* info_list;
  double* recbuf;                // [M, 8] the members' 64-byte records (kSubRecDoubles)
  int tree_barrier;              // 1: two-level arrival + release word; 0: round 4's flat counter
  unsigned int* bar;             // [0] arrival counter, [1] error flag, [2] release word, [16 + 16 g] group counters (zeroed per launch)
  unsigned int* host_err;        // pinned host word raised on a timeout: the next call reads it without a copy
  unsigned long long timeout_ticks;
  unsigned long long* stamps;    // null, or [P][5] wall-clock stamps of workgroup 0 in the launch's last iteration
  int stamp_wg = 0;              // the workgroup that writes the stamps (OSG_CFR_SUB_STAMPS = its index + 1)
  // Forest form (round 5): when there are more deal subtrees than resident workgroups (3-player leduc: 336 on 256), the
  // tree is cut ONE LEVEL DEEPER into pieces (the children of the deal roots) and the pieces are packed into one bin
  // per workgroup, balanced by size: "subtree g" above is then a forest of pieces in level order, every workgroup
  // sweeps ONE forest per pass and none takes two while the others wait.  The deal roots ("upper" histories) belong to
  // no forest: their policy rows ride in the forests' LDS rows (path codes), the pieces' root values leave through
  // root_value, and an upper member's terms are formed by the fold from those values (skip word = 2 + its index).
  const int32_t* nroot = nullptr;     // [G] piece roots of the forest; null: the bins are whole subtrees
  const int32_t* root_loc = nullptr;  // [G, NR] local index of piece root r
  const int32_t* root_idx = nullptr;  // [G, NR] its slot in root_value
  int NR = 0;
  double* root_value = nullptr;       // [histories of the pieces' level] the updating player's value of every piece root
  const int32_t* upper_rec = nullptr; // [U, 8] first child's slot in root_value, info * A, actions, 0, chance product (lo, hi), 0, 0
  // Round 5: what a pass does not have to fetch again.  The decision rows of a bin are ordered by acting player
  // (dec_off), so with one bin per workgroup (keep_rows) the policy rows STAY in LDS between passes and a pass fetches
  // only the rows the previous pass's fold rewrote (the previous updating player's) and the upper parents' rows; the
  // outcome probabilities of the bin's chance histories sit in LDS too (chance_prob: no trip to memory inside the level
  // loop); the fold takes its infostates from a packed descriptor (fold_info) in shares balanced by members (fold_off).
  const int32_t* dec_off = nullptr;   // [G, P + 2] rows of player q: [dec_off[q], dec_off[q + 1]); upper parents' rows from dec_off[P] to dec_off[P + 1]
  const double* chance_prob = nullptr;// [G, NCP] outcome probabilities of the bin's chance histories (aux = offset of the first)
  int NCP = 0;                        // (even)
  int keep_rows = 0;
  int lds_doubles = 0;                // dynamic LDS of the launch, in doubles: [policy rows ND * A | chance NCP | values NL | spare]
  const int32_t* fold_info = nullptr; // [infostates in info_list order, 4] infostate, actions, first member, members
  const double* term_val = nullptr;   // [G, P, NL] player q's return at every terminal history of the bin, local order (0 elsewhere)
  int prefetch = 1;                   // 0: nothing is fetched in the barriers' windows (measurement)
  const int32_t* fold_off = nullptr;  // [P, grid + 1] the share of workgroup w in pass q: entries [fold_off[q][w], fold_off[q][w + 1])
  // CFR-BR pass sets (k_cfr_sub<., kBr>, round 6): every infostate's best-response action index and acting player
  const int32_t* br_best = nullptr;   // [I] (null: plain CFR)
  const int32_t* br_player = nullptr; // [I]
};
OSG_D double readlane_f64(double v, int lane) {   // lane is wave-uniform: two v_readlane_b32, no LDS permute
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane(static_cast<int>(b), lane), hi = __builtin_amdgcn_readlane(static_cast<int>(b >> 32), lane);
  return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}
OSG_D void store_through_i32(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
OSG_D int32_t load_through_i32(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 16-byte written-through stores / bypassing loads (buffer instructions with the sc1 bit: what the 8-byte agent-scope
// atomics above compile to, four words at a time; the compiler keeps the wait counters)
typedef unsigned int osg_u4 __attribute__((ext_vector_type(4)));
typedef double osg_d2 __attribute__((ext_vector_type(2)));
constexpr int kCachePolicySc1 = 16;
OSG_D __amdgpu_buffer_rsrc_t through_buffer(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7FFFFFFF, 0x00020000);
}
OSG_D void store_through16(__amdgpu_buffer_rsrc_t r, unsigned int byte_off, osg_d2 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(osg_u4, v), r, static_cast<int>(byte_off), 0, kCachePolicySc1);
}
OSG_D osg_u4 load_through16(__amdgpu_buffer_rsrc_t r, unsigned int byte_off) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, static_cast<int>(byte_off), 0, kCachePolicySc1);
}
struct EvalArrays {
  const int32_t* path_off;   // [M+1]
  const int32_t* path;
  const int32_t* info_level; // [I] tree level of the infostate's member histories
  const int32_t* mem_index;  // [H] member position m of a decision history, else -1
  int M;
  double* value;             // [H, P] scratch
  double* brv;               // [H] scratch
  double* cf;                // [M] scratch
  int32_t* best;             // [I] scratch: chosen action index
  double* out;               // [2P]: ev[P] then br[P]
  double* keep = nullptr;    // [H] or null: the best-response value of EVERY history for responder keep_r
  int keep_r = -1;           //          (TabularBestResponse::Value(history), best_response.h:127-128)
};

// ---------------------------------------------------------------------------
// The best response of every player to `pol` by ONE workgroup (best_response.cc:194-227), level-synchronous: the second
// half of k_policy_eval (osg_cfr_eval.hip, where the phases are described) and the first half of every iteration of
// k_xfp_small (osg_cfr_xfp.hip).  Leaves every infostate's chosen action index in ea.best, the responders' values of the
// root in ea.out[P ...]; ea.brv [H] and ea.cf [M] are scratch, and so may pol, brv, cf and best be LDS.
// ---------------------------------------------------------------------------
OSG_D void policy_eval_best_responses(const Tree& t, const EvalArrays& ea, const double* pol) {
  const int P = t.P, A = t.A;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int r = 0; r < P; ++r) {
    for (int m = tid; m < ea.M; m += nt) {
      const int h = t.mem[m];
      if (t.actor[h] != r) continue;
      double cf = 1.0;
      for (int e = ea.path_off[m]; e < ea.path_off[m + 1]; ++e) {
        const int code = ea.path[e];
        const int slot = (code >> 24) & 0xF, idx = code & 0x7FFFFF;
        const double pr = ((code >> 23) & 1) ? t.edge_prob[idx] : (slot == r ? 1.0 : pol[idx]);
        cf = cf * pr;
      }
      ea.cf[m] = cf;
    }
    __syncthreads();
    for (int l = t.D - 1; l >= 0; --l) {
      for (int i = tid; i < t.I; i += nt) {
        if (t.info_player[i] != r || ea.info_level[i] != l) continue;
        const int n = t.nact[i];
        int best = -1;
        double best_v = -1.7976931348623157e308;  // numeric_limits<double>::lowest()
        for (int a = 0; a < n; ++a) {
          double v = 0.0;
          for (int m = t.mem_off[i]; m < t.mem_off[i + 1]; ++m)
            v += ea.cf[m] * ea.brv[t.first_child[t.mem[m]] + a];
          if (v > best_v) { best_v = v; best = a; }
        }
        ea.best[i] = best < 0 ? 0 : best;
      }
      __syncthreads();
      for (int h = t.level_off[l] + tid; h < t.level_off[l + 1]; h += nt) {
        const int k = t.kind[h];
        double v = 0.0;
        if (k == kTerminalNode) {
          v = t.term_ret[h * P + r];
        } else {
          const int fc = t.first_child[h], nc = t.nchild[h];
          if (k == kDecisionNode && t.actor[h] == r) {
            v += 1.0 * ea.brv[fc + ea.best[t.info[h]]];
          } else {
            const int row = k == kDecisionNode ? t.info[h] * A : 0;
            for (int a = 0; a < nc; ++a) {
              const double pr = k == kChanceNode ? t.edge_prob[fc + a] : pol[row + a];
              v += pr * ea.brv[fc + a];
            }
          }
        }
        ea.brv[h] = v;
      }
      __syncthreads();
    }
    if (tid == 0) ea.out[P + r] = ea.brv[0];
    if (ea.keep && r == ea.keep_r)
      for (int h = tid; h < t.H; h += nt) ea.keep[h] = ea.brv[h];
    __syncthreads();
  }
}

struct EvalJobs {
  int J, L, G, NT;            // jobs, cut level, subtrees (= histories on level L), histories on levels 0..L
  const int32_t* job;         // [J, 8] kind (0 expected returns, 1 + r best response of r), node_off, nodes, info_off,
                              //        infos, mem_off, members, -
  const int32_t* level_off;   // [J, D + 1] the job's histories of a level: a range of job-local indices
  const int32_t* node_desc;   // per job history: kind | nchild << 2 | (actor + 1) << 10
  const int32_t* node_fc;     //   job-local index of its first child
  const int32_t* node_row;    //   info * A of a decision node
  const int32_t* node_glob;   //   its index in the whole tree
  const int32_t* info_ent;    // per job infostate [4]: id, level, offset of its first member in the job's member list, members
  const int32_t* mem_ent;     // per job member [2]: member index m (position in Tree::mem), job-local history
  double* deal;               // expected returns [G, P], then best-response values [P, G]
  unsigned int* ticket;       // zero between launches
};

OSG_D void add_f64(double* p, double v) { unsafeAtomicAdd(p, v); }  // hardware fp64 atomic (LDS and L2)
// The counter stream of an external-sampling trajectory by where the walk is (level = traverser nodes above, 0 .. 2).
OSG_HD uint64_t es_stream(int level, int b1, int b2) {
  return level == 0 ? 0u : (level == 1 ? 1u + static_cast<uint64_t>(b1) : 16u + 8u * static_cast<uint64_t>(b1) + static_cast<uint64_t>(b2));
}

struct ResidentTree {
  const uint2* rec;      // [H]
  const double* uret;    // [K, P] distinct Returns() vectors
  const double* uprob;   // [nprob] distinct chance probabilities
  int K, nprob;
  int tree_global;       // 1: the traversals read the records from `rec` itself (read-only, L2-resident) and LDS holds
                         // the tables only, so that two workgroups fit a CU (leduc: 67 KB instead of 143 KB); 0: staged in LDS
};

constexpr int kMaxOsDepth = 32;

struct MmdState;   // magnetic mirror descent's host-built arrays and parameters (osg_cfr_mmd.hip)

// ---------------------------------------------------------------------------
// What the solver holds per kernel family: the plan's sizes and the device arrays a build_* function uploaded.  Each
// owns its memory (osg_device_buffer.h); the matching view struct above is formed from it by ONE function, declared
// at the end of this header (split_tree_of, sub_tree_of, eval_jobs_of, eval_arrays_of).
// ---------------------------------------------------------------------------
struct SplitPlan {   // one workgroup per deal subtree (k_cfr_split): build_split -> split_tree_of
  bool ok = false, br_ok = false;
  int G = 0, L = 0, NL = 0, NM = 0, NI = 0, threads = 0;
  size_t lds_bytes = 0;
  DeviceArray<int32_t> nloc, desc, fc, row, glob, mem_m, mem_hloc, info;
  DeviceArray<double> terms;
  DeviceArray<unsigned int> bar;
};

struct SubPlan {   // one cooperative launch, a workgroup per deal subtree of any size (k_cfr_sub): build_sub -> sub_tree_of
  bool ok = false;
  bool br_ok = false;           // k_cfr_sub<., kBr> (the CFR-BR pass set) fits the same grid
  bool dcfr_ok = false;         // k_cfr_sub<., false, kDcfr> (Discounted CFR) fits the same grid
  int G = 0, L = 0, NL = 0, K = 0, grid = 0;
  size_t lds_bytes = 0;
  int ND = 0, PL = 0;
  DeviceArray<int32_t> ndec, dec_row, rec, nloc, desc, fc, aux, mem_off, info_off, info_list;
  DeviceArray<unsigned int> bar;
  // forest form (SubTree's comment): the kernel's own skip words, piece roots, upper members
  bool forest = false;
  int NR = 0, G0 = 0;   // G0: the deal subtrees; G: the bins they (or their pieces) were packed into
  DeviceArray<unsigned long long> stamps;   // profiling stamps, made at the first call that asks for them (per solver: never shared across contexts / devices)
  DeviceArray<double> recbuf, chance_prob, term_val;
  DeviceArray<int32_t> dec_off, fold_info, fold_off;
  int NCP = 0;
  bool keep_rows = false;
  DeviceArray<int32_t> nroot, root_loc, root_idx, upper_rec;
  DeviceArray<double> root_value;
};

struct EvalPlan {   // policy evaluation (k_policy_eval, k_geval_*): eval_arrays_of, eval_policy_slot
  DeviceArray<int32_t> info_level, mem_index, best;
  DeviceArray<double> scratch;   // value [H,P] | brv [H] | cf [M] | out [2P] | policy [I,A]: laid out by eval_arrays_of alone
  PinnedArray<double> h_out;     // mapped: the evaluation kernels write their [2 P] results here
  // the large-tree evaluation's plan (launch_grid_eval), built at its first use
  DeviceArray<double> ev;             // [H, P]: the expected returns, made at the first evaluation that wants them
  std::vector<int32_t> level_off;     // [D + 1] the infostates of level l: level_info[level_off[l] ...); empty: not built
  DeviceArray<int32_t> level_info;
  DeviceArray<int32_t> d_level_off;   // the same offsets on the device (k_geval_persist)
  DeviceArray<unsigned int> bar;      // its grid barrier's counters
  int grid = 0;                       // its resident grid (0: not asked for yet, -1: none, a launch per level and phase instead)
};

struct JobsPlan {   // the evaluation as independent jobs over the device (k_eval_jobs): build_eval_jobs -> eval_jobs_of
  bool ok = false;
  int J = 0, L = 0, G = 0, NT = 0, threads = 0;
  size_t lds_bytes = 0;
  DeviceArray<int32_t> job, level, desc, fc, row, glob, info, mem;
  DeviceArray<double> deal;
  DeviceArray<unsigned int> ticket;
};

struct ResidentPlan {   // LDS-resident MCCFR traversal (k_mccfr_resident): build_resident_tree
  bool ok = false;
  size_t lds_bytes = 0;
  int n_uret = 0, n_uprob = 0;
  DeviceArray<uint64_t> rec;
  DeviceArray<double> uret, uprob;
};

struct PopulationPlan {   // payoff-tensor cells and policy aggregation (osg_cfr_population.hip): built at the first call
  bool built = false;
  int T = 0;                        // terminal histories
  int compute_units = 0;            // of the context's device
  DeviceArray<int32_t> term_seq;    // [T, P] the plan index of player p's last action on the terminal's root path, -1: none
  DeviceArray<double> term_chance;  // [T] the product of the chance probabilities on it
  DeviceArray<double> term_ret;     // [T, P] Returns()
  // grow-only, bounded by the limits the entry points state
  DeviceArray<double> plans;        // [K, I, A] the realization plan of every table of the call
  DeviceArray<double> tables;       // on_host calls: the caller's stack, weights and profiles on the device, and the results
  DeviceArray<double> weights;
  DeviceArray<int32_t> profiles;
  DeviceArray<double> out;
  DeviceArray<unsigned int> refused;   // [1] raised by a call's checking kernel: the kernels behind it write nothing
  PinnedArray<unsigned int> h_refused; // mapped: the same, kept until the next population call reports it
};

struct EfrPlan {   // extensive-form regret minimization (osg_cfr_efr.hip): built by osg_efr_set_deviations
  bool active = false;
  int form = 0;                  // 0: chosen by tree size, 1: one workgroup runs a whole call, 2: a launch per phase, level and depth
  EfrTables tables;              // the host's copy (osg_efr_deviations, osg_efr_sizes)
  DeviceArray<int32_t> dev_off, dev_info, dev_desc, nkeys, own_len, own_info, mown, depth_off, depth_info;
  DeviceArray<uint32_t> dev_cols;
  DeviceArray<int8_t> key_desc;
  DeviceArray<double> state;     // R [Dtot] | y [I, kEfrMaxKeys]: with the policy tables and the counter, the checkpoint
  DeviceArray<double> work;      // counterfactual reach [M] | own reach [M] | the policy pass's row per member [M, A]
  DeviceArray<int32_t> flags;    // live [M] | visited [I]
  size_t state_doubles(int I) const { return tables.dev_info.size() + static_cast<size_t>(I) * kEfrMaxKeys; }
};

}  // namespace osg_cfr_impl

using namespace osg_cfr_impl;

// The solver object.  It owns every device and pinned allocation it uses, through the members below: osg_cfr_destroy
// deletes it and nothing else frees solver memory.
struct osg_cfr {
  osg_cfr();
  ~osg_cfr();   // (out of line: MmdState is complete in osg_cfr_mmd.hip only)
  osg_ctx* ctx = nullptr;
  GameSpec spec;
  osg_cfr_cfg cfg{};
  int P = 0, H = 0, I = 0, A = 0, D = 0;
  int64_t n_chance = 0, n_decision = 0, n_terminal = 0;
  int max_level_width = 0;
  int average_type = 0;  // ES-MCCFR AverageType: 0 kSimple, 1 kFull (external_sampling_mccfr.h:48)
  int iteration = 0;
  // Discounted CFR (osg_cfr_set_discounting): the exponents
  bool dcfr = false;
  double dcfr_alpha = 0.0, dcfr_beta = 0.0, dcfr_gamma = 0.0;
  // One value set per iteration of the latest launch, grow-only: Discounted CFR's three factors, or
  // fictitious play's averaging weight — a solver runs one of the two, never both
  std::vector<double> h_iter_table;
  DeviceArray<double> d_iter_table;
  const char* last_kernel = "";  // the kernel family the last iterate / sample call launched (osg_cfr_last_kernel)
  // host tree
  std::vector<int32_t> level_off, parent, first_child, info, mem_off, mem, nact, legal;
  std::vector<uint8_t> kind, nchild, aidx;
  std::vector<int32_t> edge_action;  // [H] the action (or chance outcome) on the edge from the parent, -1 at the root
  std::vector<int8_t> actor, info_player;
  std::vector<double> edge_prob, term_ret;
  std::vector<std::string> keys;
  // device tree
  DeviceArray<int32_t> d_level_off, d_parent, d_first_child, d_info, d_mem_off, d_mem, d_nact;
  DeviceArray<uint8_t> d_kind, d_nchild, d_aidx;
  DeviceArray<int8_t> d_actor, d_info_player;
  DeviceArray<double> d_edge_prob, d_term_ret;
  // device tables and work arrays
  DeviceArray<double> d_tables;  // regrets | cum | cur | dreg | dpol, each [I, A]
  DeviceArray<double> d_reach;   // [H, P+1]; between CFR launches its borrowers take it through the *_in_reach accessors below
  DeviceArray<double> d_value;   // [H, P]
  bool lds_resident = false;
  size_t lds_bytes = 0;
  // small-tree kernel: root paths of the decision histories (member order)
  std::vector<int32_t> path_off, path;
  DeviceArray<int32_t> d_path_off, d_path;
  bool small_tree = false;   // the all-in-LDS variant fits
  bool path_kernel = false;  // the path-based kernel (k_cfr_small) is usable at all
  int max_path_decisions = 0;  // the most decision entries any member's root path holds
  int first_decision_level = 0;  // the first level with a decision history (SmallTree::L0)
  size_t small_lds_bytes = 0;
  std::vector<int32_t> meta32, info_player32;
  DeviceArray<int32_t> d_meta32, d_info_player32, d_skip;
  DeviceArray<double> d_node_delta;  // dreg [M, A] | dpol [M, A]
  DeviceArray<double> d_spare_delta[2];  // osg_mccfr_spare_delta_buffer: [2, I, A] each, allocated on request
  bool delta_clean[3] = {false, false, false};    // the internal / spare delta buffers are all zero (the last fold left them so)
  DeviceArray<unsigned long long> d_mccfr_stamps;   // profiling stamps of the MCCFR kernels, made at the first call that asks for them
  PinnedArray<unsigned int> h_sub_err;   // mapped: raised by a kernel when a grid barrier times out
  SplitPlan split;
  SubPlan sub;
  std::vector<int32_t> info_level, mem_index;
  bool eval_ok = true;  // every infostate's members sit on one tree level
  EvalPlan eval;
  EvalForm last_eval_form = EvalForm::kOneWorkgroup;   // launch_policy_eval's record; it names last_eval_kernel from it
  const char* last_eval_kernel = "";
  JobsPlan jobs;
  ResidentPlan resident;
  // the context's device, asked once by osg_cfr_create: what every planner and launch sizes itself by
  int num_cus = 0;
  size_t lds_optin_bytes = 0;   // dynamic LDS a workgroup may opt in to
  bool cooperative_launch = false;
  // per-infostate action values (osg_cfr_qvalues.hip): the results of a call, allocated at the first one
  DeviceArray<double> d_qv_out;
  DeviceArray<int32_t> d_qv_best;
  PopulationPlan population;
  // magnetic mirror descent (osg_cfr_mmd.hip): built at the first osg_mmd_* call
  std::unique_ptr<MmdState> mmd;
  EfrPlan efr;
  // Deep CFR (osg_deep_cfr.hip): the legal ids, the launch's strategy table and the staged rows of the last
  // osg_deep_cfr_traverse, built at the first call (a DeepState; its deleter comes with the pointer)
  std::shared_ptr<void> deep;
  // NFSP (osg_nfsp.hip): the legal ids, the row bounds and the staged rows of the last osg_nfsp_collect (an NfspState)
  std::shared_ptr<void> nfsp;

  Tree tree() const {
    Tree t;
    t.H = H; t.I = I; t.A = A; t.P = P; t.D = D;
    t.level_off = d_level_off; t.parent = d_parent; t.first_child = d_first_child; t.kind = d_kind;
    t.nchild = d_nchild; t.aidx = d_aidx; t.actor = d_actor; t.info = d_info; t.edge_prob = d_edge_prob;
    t.term_ret = d_term_ret; t.mem_off = d_mem_off; t.mem = d_mem; t.nact = d_nact; t.info_player = d_info_player;
    return t;
  }
  HostTree host_tree() const {   // what the planners of osg_cfr_plan.h read
    HostTree t;
    t.H = H; t.I = I; t.A = A; t.P = P; t.D = D; t.M = static_cast<int>(mem.size());
    t.level_off = level_off.data(); t.parent = parent.data(); t.first_child = first_child.data(); t.kind = kind.data();
    t.nchild = nchild.data(); t.aidx = aidx.data(); t.actor = actor.data(); t.info = info.data(); t.mem_off = mem_off.data();
    t.mem = mem.data(); t.nact = nact.data(); t.info_player = info_player.data(); t.edge_prob = edge_prob.data();
    t.term_ret = term_ret.data(); t.path_off = path_off.data(); t.path = path.data(); t.info_level = info_level.data();
    return t;
  }
  // Replicas: B independent solvers of the same tree (tables [B][5][I, A]); `selected` is the one the
  // table accessors / evaluation look at.
  int B = 1, selected = 0;
  size_t replica_stride() const { return 5 * static_cast<size_t>(I) * A; }
  double* replica_base(int r) const { return d_tables + static_cast<size_t>(r) * replica_stride(); }
  double* regrets() const { return replica_base(selected); }
  double* cum() const { return replica_base(selected) + static_cast<size_t>(I) * A; }
  double* cur() const { return replica_base(selected) + 2 * static_cast<size_t>(I) * A; }
  double* dreg() const { return replica_base(selected) + 3 * static_cast<size_t>(I) * A; }
  double* dpol() const { return replica_base(selected) + 4 * static_cast<size_t>(I) * A; }
};

namespace osg_cfr_impl {
// ---------------------------------------------------------------------------
// The kernels' views of the solver, each formed in one place.
// ---------------------------------------------------------------------------
// The block size of the one-workgroup kernels that sweep the tree level by level: the widest level, in whole waves.
inline int level_threads(const osg_cfr* s) { return std::max(64, std::min(((s->max_level_width + 63) / 64) * 64, 1024)); }

inline SmallTree small_tree_of(const osg_cfr* s) {   // (L0 is set by the one kernel that reads it: cfr_small_iterate)
  return SmallTree{s->d_path_off, s->d_path, static_cast<int>(s->mem.size()), static_cast<int>(s->path.size())};
}

inline SplitTree split_tree_of(const osg_cfr* s) {
  const SplitPlan& p = s->split;
  return SplitTree{p.G, p.L, p.NL, p.NM, p.NI, p.nloc, p.desc, p.fc, p.row, p.glob, p.mem_m, p.mem_hloc, p.info,
                   p.terms, p.bar, s->h_sub_err};
}

// The evaluation's scratch, EvalPlan::scratch: value [H, P] | brv [H] | cf [M] | out [2 P] | policy [I, A].  `out` is the
// device slot (CFR-BR, XFP); the evaluation proper points it at the pinned result words instead.
inline EvalArrays eval_arrays_of(const osg_cfr* s) {
  const size_t M = s->mem.size();
  EvalArrays ea;
  ea.path_off = s->d_path_off; ea.path = s->d_path; ea.info_level = s->eval.info_level; ea.mem_index = s->eval.mem_index;
  ea.M = static_cast<int>(M);
  ea.value = s->eval.scratch;
  ea.brv = ea.value + static_cast<size_t>(s->H) * s->P;
  ea.cf = ea.brv + s->H;
  ea.out = ea.cf + M;
  ea.best = s->eval.best;
  return ea;
}
inline double* eval_policy_slot(const osg_cfr* s) { return eval_arrays_of(s).out + 2 * s->P; }
inline size_t eval_scratch_doubles(const osg_cfr* s) {
  return static_cast<size_t>(s->H) * (s->P + 1) + s->mem.size() + 2 * s->P + static_cast<size_t>(s->I) * s->A;
}

// d_reach ([H, P + 1] doubles) is the CFR kernels' own between their launches only; outside them three callers borrow
// it as scratch.  Each states what it needs of the buffer here, next to the others:
//   fictitious play: avg reach [I] | best-response reach [I]        2 I <= H (P + 1): checked, the call is refused
//   action values:   the members' reaches [M, P + 1]                M <= H: holds always (a member is a history)
//   evaluation:      the responder's value of every history [H]     H <= H (P + 1): holds always
inline int xfp_reach_in_reach(const osg_cfr* s, const std::string& who, double** out) {
  if (2 * static_cast<size_t>(s->I) > static_cast<size_t>(s->H) * (s->P + 1))
    return set_error(OSG_ERR_UNSUPPORTED, who + ": more information states than the reach buffer holds");
  *out = s->d_reach;
  return OSG_OK;
}
inline double* member_reach_in_reach(const osg_cfr* s) { return s->d_reach; }
inline double* history_values_in_reach(const osg_cfr* s) { return s->d_reach; }

inline GridCfr grid_cfr_of(const osg_cfr* s, Tables tb) {   // (pol: the current policy; CFR-BR points it at its effective one)
  const size_t M = s->mem.size();
  GridCfr g;
  g.t = s->tree(); g.path_off = s->d_path_off; g.path = s->d_path; g.meta = s->d_meta32;
  g.info_player = s->d_info_player32; g.value = s->d_value; g.dreg = s->d_node_delta;
  g.dpol = s->d_node_delta + M * s->A; g.skip = s->d_skip; g.tb = tb; g.M = static_cast<int>(M);
  g.pol = tb.cur;
  return g;
}

// ---- Which form serves a call (DESIGN.md section 6 has the table).  Both switches are read at every call. ----
// Trees beyond one workgroup's reach (and too large for the jobs) are evaluated with a launch per level and phase
// (k_geval_*); OSG_EVAL_GRID=1 forces that form, 0 forbids it (the tests compare the three).
inline bool eval_grid_on(const osg_cfr* s) {
  const char* e = getenv("OSG_EVAL_GRID");
  if (e && e[0] == '0') return false;
  if (e && e[0] == '1') return true;
  return s->H > 65536;
}
// The evaluation, best responses and history values, the action values' responder pre-pass, CFR-BR: osg_cfr_cfg.kernel has
// no say.  OSG_EVAL_JOBS=0 keeps the one-workgroup evaluation for trees that could take the jobs.
inline EvalForm eval_form(const osg_cfr* s, bool jobs_allowed = true) {
  const char* e = getenv("OSG_EVAL_JOBS");
  if (jobs_allowed && s->jobs.ok && !(e && e[0] == '0')) return EvalForm::kJobs;
  return eval_grid_on(s) ? EvalForm::kGrid : EvalForm::kOneWorkgroup;
}
// Fictitious play's best responses: GRID forces the launches per level and phase, GENERAL and PATH forbid the jobs.
inline EvalForm eval_form_for_kernel_option(const osg_cfr* s) {
  const int k = s->cfg.kernel;
  return k == OSG_CFR_KERNEL_GRID ? EvalForm::kGrid : eval_form(s, k != OSG_CFR_KERNEL_GENERAL && k != OSG_CFR_KERNEL_PATH);
}
// The action values' own pass (k_qv_* per level, or k_qvalues_small): the jobs have no say.
inline bool action_values_take_the_grid(const osg_cfr* s) { return s->cfg.kernel == OSG_CFR_KERNEL_GRID || eval_grid_on(s); }
// osg_cfr_iterate.  Trees far beyond one workgroup: full-grid launches per phase (GRID forces them), or where the tree has
// the shape the persistent cooperative launch with a workgroup per deal subtree (SUB forces it).
inline CfrForm cfr_iterate_form(const osg_cfr* s) {
  const int k = s->cfg.kernel;
  const bool grid = s->path_kernel && s->B == 1 && (k == OSG_CFR_KERNEL_GRID || (k == OSG_CFR_KERNEL_AUTO && s->H > 65536));
  const bool sub = s->sub.ok && (!s->dcfr || s->sub.dcfr_ok) && s->B == 1 && (k == OSG_CFR_KERNEL_SUB || (k == OSG_CFR_KERNEL_AUTO && grid));
  if (sub || grid) return sub ? CfrForm::kSub : CfrForm::kGrid;
  return s->split.ok && (k == OSG_CFR_KERNEL_AUTO || k == OSG_CFR_KERNEL_SPLIT) ? CfrForm::kSplit : CfrForm::kSmall;
}
// osg_cfr_br_iterate's passes.  Large trees (their best responses take the grid): the P passes in ONE persistent launch per
// iteration (GRID keeps a launch per phase: the cross-check).
inline CfrForm cfr_br_iterate_form(const osg_cfr* s) {
  const int k = s->cfg.kernel;
  if (s->split.ok && s->split.br_ok && (k == OSG_CFR_KERNEL_AUTO || k == OSG_CFR_KERNEL_SPLIT)) return CfrForm::kSplit;
  if (eval_form(s) != EvalForm::kGrid || !s->path_kernel) return CfrForm::kSmall;
  return s->sub.ok && s->sub.br_ok && k != OSG_CFR_KERNEL_GRID ? CfrForm::kSub : CfrForm::kGrid;
}

// ---- osg_cfr.hip ----
int cfr_sub_error(const osg_cfr* s);   // a grid barrier timed out in an earlier launch: the solver refuses further work
void discount_factors(double alpha, double beta, double gamma, int iteration, double out[3]);
// The factor table of iterations iteration0 + 1 ... iteration0 + iters on the device (null where the solver does not discount).
int cfr_discount_table(osg_cfr* s, int iteration0, int iters, const double** d_table);
// ---- osg_cfr_small.hip ----
void cfr_small_prepare(osg_cfr* s);    // LDS caps of k_cfr<true> / k_cfr_small (clears lds_resident / small_tree where refused)
int cfr_small_iterate(osg_cfr* s, Tables tb, int iters, unsigned grid_b);   // k_cfr_small / k_cfr
void cfr_general_br_pass(osg_cfr* s, Tables tb, osg_cfr_cfg cfg);           // k_cfr<false, kBr> x 1
// ---- osg_cfr_split.hip ----
int build_split(osg_cfr* s);
int launch_split(osg_cfr* s, SmallTree stree, SplitTree sp, Tables tb, int iters, int iteration0, osg_cfr_cfg cfg, bool br,
                 const double* disc = nullptr);
// ---- osg_cfr_sub.hip ----
int build_sub(osg_cfr* s);
SubTree sub_tree_of(const osg_cfr* s);   // reads the OSG_CFR_SUB_* switches, at every call
int cfr_sub_iterate(osg_cfr* s, Tables tb, int iters);      // k_cfr_sub
int cfr_grid_iterate(osg_cfr* s, Tables tb, int iters);     // k_gcfr_*
// CFR-BR on large trees: a launch per phase / k_cfr_sub<., kBr>; `ef`: the form of their best responses
int cfr_grid_br_iterate(osg_cfr* s, Tables tb, EvalForm ef, const EvalArrays& ea, osg_cfr_cfg cfg, int iters);
int cfr_sub_br_iterate(osg_cfr* s, Tables tb, EvalForm ef, const EvalArrays& ea, osg_cfr_cfg cfg, int iters);
// ---- osg_cfr_eval.hip ----
int build_eval_jobs(osg_cfr* s);
EvalJobs eval_jobs_of(const osg_cfr* s);
// One evaluation's launches in the form given, no wait and no copy: of the policy `src`, or (from_cum) of the cumulative
// table's normalisation; only_br: the best responses alone, for CFR-BR and fictitious play.  Sets last_eval_form.
int launch_policy_eval(osg_cfr* s, EvalForm form, const EvalArrays& ea, const double* src, bool from_cum, double* d_pol, bool only_br);
// ---- osg_cfr_mccfr.hip ----
int build_resident_tree(osg_cfr* s);
// ---- osg_cfr_mmd.hip ----
bool mmd_mode(const osg_cfr* s);       // osg_mmd_set_params was accepted: pi and avg_x live in the cur and cum tables
int mmd_after_reset(osg_cfr* s);       // avg_x = x of the fresh uniform policy
// ---- osg_deep_cfr.hip ----
int deep_supported(const osg_cfr* s, const char* who);   // what Deep CFR and NFSP serve: rows of at most 4 action ids, every id below the width
bool reservoir_serves(const osg_reservoir* b, const osg_cfr* s);   // the solver's row width and context
// m sequential appends of device rows, in row order (osg_reservoir_append without its argument checks)
int reservoir_append(osg_reservoir* b, int64_t m, const int32_t* d_info, int32_t iteration, const float* d_values);
// ---- osg_cfr_efr.hip ----
bool efr_mode(const osg_cfr* s);       // osg_efr_set_deviations was accepted
int efr_after_reset(osg_cfr* s);       // R and y back to 0
}  // namespace osg_cfr_impl
