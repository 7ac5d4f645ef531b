/* =============================================================================
 * osg_abi.h — C-ABI of the MI355X batched game-step and search engine.
 *
 * This is the drop-in boundary for OpenSpiel's data-parallel hot path: every
 * entry point below is what a binding of the reference (pybind / cgo / Rust
 * FFI) would call instead of looping over per-state virtual calls.  Plain
 * pointers and sizes only — no torch, no C++ types.  Conventions follow the
 * reference's in-tree C API (open_spiel/rust/src/rust_open_spiel.h:18-88:
 * opaque handles, caller-supplied out-buffers).
 *
 * All functions return 0 on success and a negative osg_status on failure; the
 * message is available from osg_last_error() (thread-local).  Nothing in the
 * library calls exit() or throws across the boundary; the C++ host classes
 * (open_spiel_amd/csrc/host) turn a non-zero code into SpielFatalError so the
 * observable error behaviour matches open_spiel/spiel_utils.cc:119-137.
 *
 * Pointers named d_* are DEVICE pointers (HBM, e.g. torch tensor.data_ptr());
 * pointers named h_* are host pointers.  Buffers named without prefix take an
 * `on_host` flag.  The library owns the memory behind handles; the caller owns
 * every buffer it passes in.  An osg_ctx is bound to one device and one HIP
 * stream and is not thread-safe; distinct contexts are independent.  All work
 * is enqueued on the context's stream; functions that write to host buffers
 * synchronise that stream before returning, device-only functions do not.
 * =========================================================================== */
#ifndef OSG_ABI_H_
#define OSG_ABI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  OSG_OK = 0,
  OSG_ERR_INVALID = -1,     /* bad argument / malformed game string           */
  OSG_ERR_UNSUPPORTED = -2, /* game or parameter not available on the device   */
  OSG_ERR_HIP = -3,         /* a HIP runtime call failed                       */
  OSG_ERR_ILLEGAL = -4,     /* an illegal action was applied (count > 0)       */
  OSG_ERR_NOMEM = -5
} osg_status;

typedef struct osg_ctx osg_ctx;     /* one per (process, device): HIP stream      */
typedef struct osg_batch osg_batch; /* N states of one game, SoA in HBM           */
typedef struct osg_cfr osg_cfr;     /* a flattened game tree + fp64 CFR tables    */

/* Sentinels (open_spiel/spiel_globals.h:26-56,82). */
#define OSG_CHANCE_PLAYER (-1)
#define OSG_TERMINAL_PLAYER (-4)
#define OSG_INVALID_ACTION (-1)

/* Replaces Game::NumDistinctActions / MaxChanceOutcomes / NumPlayers /
 * ObservationTensorShape / InformationStateTensorShape / MaxGameLength /
 * MinUtility / MaxUtility (open_spiel/spiel.h:927-1255). */
typedef struct {
  int32_t game_kind;           /* 0 ttt, 1 connect_four, 2 hex, 3 kuhn, 4 leduc */
  int32_t num_players;
  int32_t num_distinct_actions;
  int32_t max_chance_outcomes;
  int32_t max_game_length;
  int32_t max_chance_nodes;
  int32_t obs_size;            /* ObservationTensorSize()                        */
  int32_t info_size;           /* InformationStateTensorSize(), 0 if absent      */
  int32_t obs_shape[4];        /* rank in obs_rank                               */
  int32_t obs_rank;
  int32_t info_shape[4];
  int32_t info_rank;
  int32_t mask_words;          /* u32 words per legal mask = ceil(max(A,C)/32)   */
  int32_t compact_mask_bytes;  /* bytes per state of the fused step's mask: 1,2,4*mask_words */
  int32_t state_words;         /* SoA planes per state                           */
  int32_t state_word_bytes;    /* 4 or 8: bytes per plane element                */
  double min_utility;
  double max_utility;
  char canonical[128];         /* Game::ToString(): the string as parsed         */
} osg_game_desc;

const char* osg_last_error(void);

/* ---- context ------------------------------------------------------------ */
/* own_stream != 0: the library creates (and owns) a non-blocking stream and
 * `stream` is ignored.  own_stream == 0: `stream` is a hipStream_t owned by the
 * caller (e.g. torch's current stream; NULL is the device's default stream).
 * The engine is written for one process per GPU: osg_ctx_create makes `device` the calling
 * thread's current device and later calls launch on the context's stream without selecting it
 * again — a process that holds contexts on several devices makes the context's device current
 * (hipSetDevice) on the calling thread before each call. */
int osg_ctx_create(int device, void* stream, int own_stream, osg_ctx** out);
int osg_ctx_destroy(osg_ctx* ctx);
int osg_ctx_synchronize(osg_ctx* ctx);
void* osg_ctx_stream(osg_ctx* ctx);
/* Give back what the context caches between calls: the IS-MCTS workspace (and with it the trees of the last
 * osg_ismcts_search), the MCTS node pool (grow-only otherwise: a search without a
 * node budget sizes it at 1 + max_simulations x widest-node slots per root, up to 60 % of the free HBM) and the
 * staging buffer.  Waits for the stream first.  The next search allocates again. */
int osg_ctx_trim(osg_ctx* ctx);
/* Rebind a context created on a caller's stream (own_stream == 0) to another stream of the same device, e.g. the
 * stream a hipGraph is being captured on: every later call of the context's objects is issued there. */
int osg_ctx_set_stream(osg_ctx* ctx, void* stream);

/* ---- game description (no device needed) -------------------------------- */
/* Replaces LoadGame(game_string) (open_spiel/spiel.cc:255) for the five hot-path
 * games; unknown parameters / wrong types are OSG_ERR_INVALID as in
 * spiel.cc:65-90, games or sizes without a device layout OSG_ERR_UNSUPPORTED.
 * The sizes with a layout (every accepted string equals the reference at every ply; the message of a refusal names the limit):
 *   connect_four  rows <= 127, columns <= 32, (rows + 1) * columns <= 128, and the line test's largest shift below the
 *                 width of the board's word(s): (x_in_row - 1) * (rows + 2) — 2 * (rows + 2) for x_in_row = 4 — at
 *                 most 63 where (rows + 1) * columns <= 64, at most 127 above (so 29 rows with four in a row in one
 *                 word, 61 in two; 7 x 8 up to x_in_row = 8, 7 x 16 up to 15).  Every x_in_row >= 1 otherwise: a value
 *                 above max(rows, columns), which the reference accepts and for which it never finds a line, is
 *                 played as max(rows, columns) + 1 (no line either): no kernel's trip count grows with the value given
 *   hex           num_cols <= 31 and num_cols * num_rows (+ 1 with swap) <= 384; swap only where num_cols <= num_rows,
 *                 plain_obs_tensor only on square boards (the reference indexes out of bounds elsewhere); boards with
 *                 a single row or column are served by the rules, not by the entry points that play out (osg_rollout)
 *   kuhn_poker, leduc_poker   2 to 10 players (OSG_ERR_INVALID outside, as in the reference)
 * Each dimension is checked before a product is formed: rows = 2^31 - 1 is refused, not wrapped. */
int osg_game_describe(const char* game_string, osg_game_desc* out);

/* ---- batches of states --------------------------------------------------- */
/* Replaces Game::NewInitialState() x n (spiel.h:943-950). */
int osg_batch_create(osg_ctx* ctx, const char* game_string, int64_t n, osg_batch** out);
int osg_batch_destroy(osg_batch* b);
int64_t osg_batch_size(const osg_batch* b);
int osg_batch_describe(const osg_batch* b, osg_game_desc* out);
int osg_batch_reset(osg_batch* b);                              /* all -> initial state  */
/* State::Clone() for a whole batch (spiel.h:737). Same game and size. */
int osg_batch_copy(osg_batch* dst, const osg_batch* src);
/* dst[i] = src[index[i]] (dst size = number of indices): Clone() of chosen states. */
int osg_batch_gather(osg_batch* dst, const osg_batch* src, const int64_t* index, int on_host);
/* Raw SoA image: state_words planes of n elements each (plane-major). */
int osg_batch_download(const osg_batch* b, void* h_words);
int osg_batch_upload(osg_batch* b, const void* h_words);
/* State `index` of the batch := the position with these cells, one character per cell ('.', 'x', 'o').  tic_tac_toe: 9
 * cells, cell a = action a (TicTacToeState(game, TicTacToeStateStruct), games/tic_tac_toe/tic_tac_toe.cc:273-336);
 * connect_four: rows x cols cells, cell r * cols + c with row 0 the BOTTOM row (ConnectFourStateStruct::board;
 * ConnectFourState(game, struct, strict_validation) and ConnectFourState(game, string),
 * games/connect_four/connect_four.cc:352-470).  The position is built on the device with the game's own rules
 * (outcome recomputed; player to move = parity of the stone count, which is how this layout stores it — the
 * piece-count rules of the reference's constructors are the caller's to enforce).  OSG_ERR_INVALID: wrong cell count,
 * another character, a gap in a connect_four column, both players with a line; OSG_ERR_UNSUPPORTED: other games. */
int osg_batch_set_cells(osg_batch* b, int64_t index, const char* cells, int n_cells);
/* Device pointer to the SoA planes (plane k at base + k * n elements). */
void* osg_batch_device_ptr(osg_batch* b);

/* State::LegalActionsMask() (spiel.cc:518-524), bit-packed: mask[i*W + a/32] bit a%32;
 * at chance nodes the bits are the legal chance outcomes; all zero when terminal. */
int osg_legal_mask(const osg_batch* b, uint32_t* mask, int on_host);

/* State::ApplyAction (spiel.cc:441-451 + each game's DoApplyAction), in place.
 * actions[i] == -1 leaves state i untouched.  Illegal actions (not in
 * LegalActions(), or any action on a terminal state) leave the state untouched
 * and are counted; the count is returned through *illegal (may be NULL; then a
 * non-zero count turns into OSG_ERR_ILLEGAL at the next synchronising call). */
int osg_apply(osg_batch* b, const int32_t* actions, int on_host, int64_t* h_illegal);

/* IsTerminal / CurrentPlayer / Returns (per game; e.g. connect_four.cc:122-128,
 * 277-285).  Any pointer may be NULL.  returns is [n, num_players] fp64. */
int osg_status_query(const osg_batch* b, int8_t* cur_player, uint8_t* terminal,
                     double* returns, int on_host);

/* State::ChanceOutcomes() probabilities for every outcome id: probs[n, max_chance]
 * fp64, 0 for outcomes that are not legal (or at non-chance nodes). */
int osg_chance_probs(const osg_batch* b, double* probs, int on_host);

/* The fused headline kernel: LegalActions check + ApplyAction + IsTerminal /
 * CurrentPlayer / outcome + LegalActions of the successor, one pass over the
 * SoA state.  Device pointers only; src may equal dst.
 *   d_actions [n] u8   action id (0xFF = skip)
 *   d_mask    [n * compact_mask_bytes] legal mask of the successor state; NULL = do not write it: hex boards of up
 *                      to 128 cells only (hex.cc:280-293: the successor's legal actions are its empty cells, i.e.
 *                      ~occupied of the record the step writes), OSG_ERR_UNSUPPORTED for every other game.
 *                      A caller deriving that mask from the raw words must (i) AND it with the board's cell bits — in
 *                      the folded record (hex 9x9, 11x11, 19x19: osg_game_desc.state_words == 4 planes x words, no meta
 *                      word) the top 5 bits of every plane's LAST word (bits 27-31) carry mover / result / ply / first
 *                      move, not cells: mask that word with 0x07FFFFFF — and (ii) treat a terminal state (status bit7)
 *                      as having no legal action.  osg_legal_mask does both.
 *   d_status  [n] u8   bit7 terminal | bit6 action was illegal (state unchanged) |
 *                      not terminal: bits0-3 = current player + 1 (0 = chance) |
 *                      terminal:     bits0-2 = outcome (board games: 0 p0 wins,
 *                      1 p1 wins, 2 draw; poker: 7 = see osg_status_query) */
int osg_step(const osg_batch* src, osg_batch* dst, const uint8_t* d_actions,
             void* d_mask, uint8_t* d_status);

/* State::ObservationTensor(player) / InformationStateTensor(player)
 * (spiel.cc:908-945 + each game; observer.h:174-185 zero-fill semantics).
 * which: 0 observation, 1 information state.  player in [0, P), or -1 = the
 * state's current player (player 0 where that is chance/terminal).
 * out is [n, size] fp32. */
int osg_observation(const osg_batch* b, int player, int which, float* out, int on_host);

/* State::InformationStateString(player) of state `index` (kuhn_poker.cc:109-166,
 * leduc_poker.cc:198-239) — the key of the CFR tables.  Host formatter over the packed
 * state words; returns the length (excluding NUL) or <0. */
int osg_information_state_string(const osg_batch* b, int64_t index, int player, char* buf, int cap);

/* State::ObservationString(player) of state `index`: the board (tic_tac_toe.cc:163-175,
 * connect_four.cc:212-222, hex.cc:341-359) or the imperfect-recall observer string of the poker games
 * (kuhn_poker.cc:109-166, leduc_poker.cc:198-239).  Host formatter over the packed state words; returns
 * the length (excluding NUL) or <0. */
int osg_observation_string(const osg_batch* b, int64_t index, int player, char* buf, int cap);

/* State::ToString() of state `index` (tic_tac_toe.cc:163-175, connect_four.cc:212-222, hex.cc:341-359,
 * kuhn_poker.cc:253-268, leduc_poker.cc:463-496) and State::ActionToString(player, action)
 * (tic_tac_toe.cc:266-270, connect_four.cc:158-161, hex.cc:295-314, kuhn_poker.cc:244-251,
 * leduc_poker.cc:459-461); player -1 = chance.  Host formatters; return the length or <0. */
int osg_state_string(const osg_batch* b, int64_t index, char* buf, int cap);
int osg_action_string(const osg_batch* b, int64_t index, int player, int32_t action, char* buf, int cap);

/* Plain device-to-device copy of `bytes` (a multiple of 16; both pointers 16-byte aligned) on the
 * context's stream with 16-byte accesses per lane and non-temporal stores (the fastest plain copy measured
 * here: 91.6 us for 587 MB against 96.1 us with ordinary stores): the memory-only ceiling the step / tensor kernels
 * are measured against (bench.py `roofline.copy_ceiling`; SURVEY.md 8(d) "measured device-copy
 * bandwidth as secondary denominator").  No reference counterpart. */
int osg_copy_bytes(osg_ctx* ctx, void* d_dst, const void* d_src, int64_t bytes);

/* Environment loop on device: `steps` times { sample a uniformly random legal
 * action (chance outcomes by their distribution), apply, auto-reset terminal
 * states to the initial state }.  d_counters[0] += env steps applied,
 * d_counters[1] += episodes finished.  RNG stream = (seed, global index). */
int osg_random_steps(osg_batch* b, uint64_t seed, int64_t index_offset, int steps,
                     unsigned long long* d_counters);

/* SURVEY.md 8(d) synthetic benchmark inputs on the counter stream (seed, index_offset + i): state i = the
 * initial state advanced by depth_i = draw mod depth_mod uniformly random legal moves (chance outcomes by
 * their distribution), the trajectory re-drawn from the same stream if it ends earlier, so every state is
 * non-terminal; d_actions [n] u8 (may be NULL) = one more uniformly random legal action of that state,
 * d_depth [n] i32 (may be NULL) = depth_i.  The batch a benchmark times can therefore be regenerated by the
 * CPU oracle state for state (oracle/spiel_oracle_capi.cpp osgo_synth_batch restates the loop; the rules it
 * runs are the reference's: spiel.cc:441-451, connect_four.cc:130-156).  depth_mod in [1, MaxGameLength()];
 * a depth no trajectory survives (e.g. >= the shortest game) degrades to the initial state after 2^14 attempts.
 * No reference counterpart: the reference's benchmarks build their states one by one on the host. */
int osg_synth_batch(osg_batch* b, uint64_t seed, int64_t index_offset, int depth_mod, uint8_t* d_actions,
                    int32_t* d_depth);

/* One reinforcement-learning environment step for every state (python/rl_environment.py:379-418
 * Environment.step + get_time_step; replaces the Python loop of python/vector_env.py:51-54).
 * Device pointers only.  d_should_reset [n] u8 is in/out: an environment flagged 1 starts a new
 * episode and ignores its action; otherwise d_actions[i] is applied (-1: environment left as it is).
 * Chance nodes are then
 * resolved by sampling from the counter stream (seed, index_offset + i, step_index).
 * Outputs: d_cur_player [n] i8, d_step_type [n] u8 (0 FIRST, 1 MID, 2 LAST), d_rewards [n, P]
 * f64 (terminal returns at LAST, zeros otherwise), d_mask [n, mask_words] u32 legal mask of the
 * new state; d_should_reset becomes 1 exactly where the step type is LAST.  Illegal actions leave
 * the state unchanged and are reported by osg_ctx_synchronize (OSG_ERR_ILLEGAL). */
int osg_env_step(osg_batch* b, const int32_t* d_actions, uint8_t* d_should_reset, uint64_t seed, int64_t index_offset,
                 int64_t step_index, int8_t* d_cur_player, uint8_t* d_step_type, double* d_rewards, uint32_t* d_mask);
/* The same step with compact side arrays for hosts that keep their own TimeStep layout (no reference counterpart: the
 * reference's TimeStep carries int actions and float64 rewards, python/rl_environment.py:257-318 — 20 of the 60 bytes
 * osg_env_step moves per connect_four environment; this form moves 41).  d_actions [n] u8: the action, 0xFF = leave the
 * environment as it is.  d_flags [n] u8 is in/out: bits 0-1 the step type (0 FIRST, 1 MID, 2 LAST), bits 2-7 the current
 * player + 4 (chance -1 -> 3, terminal -4 -> 0); an environment whose flag byte says LAST on input starts a new episode
 * and ignores its action (initialise the array to 2 to start every environment).  d_rewards_x2 [n, P] i8 = TWICE the
 * reward (the returns of the games served are multiples of 0.5): terminal returns at LAST, zeros otherwise; a game whose
 * doubled returns do not fit a signed byte (leduc_poker with 6+ players), or with more than 255 actions (hex from 16 x 16),
 * answers OSG_ERR_UNSUPPORTED.  d_mask, the chance
 * sampling, the counter streams and the illegal-action report are osg_env_step's: the two forms step identically. */
int osg_env_step_compact(osg_batch* b, const uint8_t* d_actions, uint8_t* d_flags, uint64_t seed, int64_t index_offset,
                         int64_t step_index, int8_t* d_rewards_x2, uint32_t* d_mask);

/* algorithms::RandomRolloutEvaluator::Evaluate (open_spiel/algorithms/mcts.cc:43-72)
 * for every root: n_rollouts uniform-random playouts to the end of the game.
 * sum_returns [n, P] fp64 = SUM over rollouts of Returns() (divide by n_rollouts
 * for Evaluate's mean); steps[n] i32 (may be NULL) = plies played.  Rollout r of
 * root i draws from the counter stream (seed, index_offset + i, r).  hex with steps == NULL: the playouts place their
 * stones with the same draws until the board is full and read the winner off the filled board (a hex game cannot be
 * un-won) — the same sums, ~5 x the rate of the move-by-move rules, which a non-NULL steps keeps.
 * A playout is cut off after 512 moves (no game served here lasts longer than 130): a record the
 * rules cannot finish — uploaded, neither terminal nor with a legal action — contributes Returns()
 * of a running game (zeros) instead of spinning on the device.  hex boards with a single row or
 * column are refused (OSG_ERR_UNSUPPORTED): with the reference's `else if` between a colour's two
 * edges (hex.cc:122-126,146-150) one colour can never win there, so playouts would not end. */
int osg_rollout(const osg_batch* roots, uint64_t seed, int64_t index_offset, int n_rollouts,
                double* sum_returns, int32_t* steps, int on_host);

/* algorithms::MCTSBot (open_spiel/algorithms/mcts.{h,cc}) for every root of the
 * batch, one wavefront per root.  Fields as MCTSBot's constructor (mcts.h:161-169).
 * The same two guards as osg_rollout apply (playout length, one-row / one-column hex boards);
 * a node that is not terminal and has no legal action is evaluated as a leaf, never expanded. */
typedef struct {
  double uct_c;
  int32_t max_simulations;
  int32_t n_rollouts;       /* RandomRolloutEvaluator(n_rollouts, seed)            */
  int32_t solve;            /* MCTS-Solver backup (mcts.cc:398-434)                */
  int32_t max_nodes;        /* > 0: MCTSBot's max_nodes_ = (max_memory_mb << 20) / sizeof(SearchNode) + 1
                               (mcts.cc:214): when a tree reaches it, every node visited fewer than
                               gc_limit_ times loses its children (GarbageCollect, mcts.cc:441-482).
                               <= 0: no caller limit: the pool gets 1 + max_simulations x widest-node slots
                               per root (it can never run out) when that fits 60 % of the free HBM, else
                               what fits, collected the same way at that size.  The pool stays cached in
                               the context (grow-only) until osg_ctx_trim / osg_ctx_destroy          */
  uint64_t seed;
  int64_t index_offset;     /* global index of root 0 (multi-GPU sharding)         */
  int32_t layout;           /* 0 auto; 1 one LANE per root (64 searches per wavefront,
                               sequential rollouts); 2 one WAVEFRONT per root (children
                               and rollouts spread over the 64 lanes; hex playouts as a
                               wave-parallel random fill).  The two layouts define their
                               random streams differently (see osg_common.h), so results
                               are reproducible per layout, not across layouts.  Layout 2
                               serves games of up to 128 actions and (round 6) the hex boards
                               above 128 cells WITHOUT the swap rule (to 19 x 19: 3 / 4 / 6
                               64-cell sets per colour in scalar registers; 0 picks it there —
                               2.1-2.6 x layout 1 on 12 x 12 ... 16 x 16); hex above 128 cells
                               with the swap rule, connect_four above 64 board bits and
                               leduc_poker with 4+ players are searched with layout 1 (0 picks
                               it), and layout 2 answers OSG_ERR_UNSUPPORTED for them.  A node
                               holds up to 511 actions.  Layout 2 is TUNED for hex without the
                               swap rule (what 0 picks it for); its instantiations for the other
                               games are correct (replay parity in the tests) but spill 76-129
                               vector registers (profiles/r05_kernel_resources.txt): use layout 1
                               for tic_tac_toe, connect_four, kuhn_poker and leduc_poker      */
  int32_t child_selection_policy;  /* ChildSelectionPolicy (mcts.h:148): 0 UCT (mcts.cc:90-101),
                               1 PUCT (mcts.cc:103-112) with the evaluator's prior — uniform over
                               the legal actions for RandomRolloutEvaluator (mcts.cc:74-87)        */
} osg_mcts_cfg;
/* Outputs (host or device by on_host; any may be NULL):
 *   best_action [n] i32            SearchNode::BestChild().action (mcts.cc:127-143)
 *   child_visits [n, A] i32        explore_count of the root child for action a
 *   child_reward [n, A] f64        total_reward of that child
 *   child_outcome [n, A] i8        proven outcome for the root player (-1,0,1) or 2 = unproven,
 *                                  3 = no such child
 *   root_stats [n, 4] f64          root explore_count, nodes used, root outcome for
 *                                  the root player (NaN if unproven), simulations run */
int osg_mcts_search(const osg_batch* roots, const osg_mcts_cfg* cfg, int32_t* best_action,
                    int32_t* child_visits, double* child_reward, int8_t* child_outcome,
                    double* root_stats, int on_host);

/* algorithms::AlphaBetaSearch (open_spiel/algorithms/minimax.cc:49-137 _alpha_beta, 222-256 the entry; its Python twin
 * python/algorithms/minimax.py:26-149) for every root of the batch: one deterministic search per root, node for node
 * the reference's — children in ascending action order (LegalActions()), window (-inf, +inf) at the root
 * (minimax.cc:250-253), the maximiser replaces on child > value and the minimiser on child < value (minimax.cc:88,122),
 * cut-off on alpha >= beta (minimax.cc:95-98,129-132), the best action recorded at the root only (minimax.cc:90-92).
 * tic_tac_toe, connect_four (boards above 64 bits included) and hex of up to 128 cells, with and without swap;
 * OSG_ERR_UNSUPPORTED for kuhn_poker and leduc_poker (not deterministic: minimax.cc:232) and for larger hex boards.
 *   depth_limit        < 0: unlimited (the reference's tests pass -1); a node at depth 0 that is not terminal takes
 *                      the leaf value (minimax.cc:57-65)
 *   maximizing_player  -1: the player to move at each root (kInvalidPlayer, minimax.cc:244-246; at a terminal root,
 *                      where the reference has no player to name, the player who would be to move); 0 or 1: that
 *                      player at every root
 *   leaf_mode          the reference's value_function is a host callback; the device offers OSG_AB_LEAF_NONE (its
 *                      absence: the fatal error of minimax.cc:57-61 becomes status 1 of that root) and
 *                      OSG_AB_LEAF_CONSTANT (value_function = a constant, leaf_value) — with depth_limit D that answers
 *                      "can the maximiser force a result within D plies?"
 *   max_nodes          > 0: node budget per root; a root that would need more stops with status 2, so no search
 *                      holds the device for longer than the caller allowed
 * OSG_ERR_INVALID: max_nodes <= 0, maximizing_player outside -1..1, an unknown leaf mode.
 * Outputs (host or device by on_host; all required), per root:
 *   value [n] f64        the reference's first result: only ever copied from the game's returns or leaf_value, bit for bit
 *   best_action [n] i32  its second; -1 (kInvalidAction) at a terminal root or at depth_limit 0
 *   nodes [n] i64        the number of _alpha_beta invocations, the root's included
 *   status [n] u8        0 done; 1 reached the depth limit with no leaf value; 2 node budget exhausted.  For a status
 *                        other than 0, value is NaN, best_action -1 and nodes unspecified. */
#define OSG_AB_LEAF_NONE 0
#define OSG_AB_LEAF_CONSTANT 1
typedef struct {
  int32_t depth_limit;
  int32_t maximizing_player;
  int32_t leaf_mode;
  double leaf_value;
  int64_t max_nodes;
} osg_ab_cfg;
int osg_alpha_beta_search(const osg_batch* roots, const osg_ab_cfg* cfg, double* value, int32_t* best_action,
                          int64_t* nodes, uint8_t* status, int on_host);

/* ---- information-set MCTS -------------------------------------------------------------------------------------
 * ISMCTSBot (python/algorithms/ismcts.py; algorithms/is_mcts.{h,cc}) with RandomRolloutEvaluator(n_rollouts) for every
 * root of a kuhn_poker or leduc_poker batch (every parameter set, 2 or 3 players): one tree per root whose nodes are keyed
 * by (player to act, InformationStateString), the root state resampled from the searcher's information state before
 * every simulation (ResampleFromInfostate's rejection loops), one child expanded per visit, and the UCT / PUCT choice
 * among the children within 1e-5 of the best.  The Python file is followed where the two differ: it draws
 * randint(len(candidates)) for a single candidate too.  All draws of root i come from ONE stream
 * Rng(seed, index_offset + i, 0), consumed in the reference's order (csrc/osg_ismcts.h lists it), so a scripted
 * random_state makes the reference's own bot build the same tree, node for node.
 *   max_world_samples  <= 0: unlimited (a fresh resample per simulation); k > 0: the first k simulations resample and keep
 *                      their sample, later ones take samples[below(k)] (ismcts.py:206-217)
 *   max_nodes          the table of each root; <= 0: as many as the search can create (one per simulation at most).  A
 *                      root that needs more stops with status 2; nothing is ever written past a table
 * OSG_ERR_UNSUPPORTED: another game, more than 3 players.  OSG_ERR_INVALID: max_simulations or n_rollouts < 1, an unknown
 * final_policy_type or child_selection_policy, max_nodes above 2^24, and a root that is a chance node or terminal (the
 * message names the first such row).
 * Outputs (host or device by on_host; any may be NULL), A = num_distinct_actions:
 *   policy [n, A] f64            get_final_policy (ismcts.py:161-204) by action; 0 for an action that is not legal
 *   sampled_action [n] i32       step_with_policy's draw: one more unit(), a CDF scan over the policy list in ITS order
 *                                (children in insertion order, then the legal actions never expanded)
 *   child_visits [n, A] i32, child_return_sum [n, A] f64     of the root's children
 *   expansion_rank [n, A] i32    the insertion rank of the action's child at the root; -1 = never expanded
 *   nodes [n] i32                nodes in the root's table
 *   status [n] u8                0 done; 1 the root was never visited (max_simulations = 1 only evaluates it: the
 *                                reference's `assert node.total_visits > 0`); 2 the table was full; 3 the record is not a
 *                                state of the game.  For a status other than 0 the policy is NaN and sampled_action -1.
 * A root with a single legal action gets policy {a: 1}, no simulation, no draw and 0 nodes (ismcts.py:117-119).
 *
 * The trees of a context's last search stay in its workspace until the next search or osg_ctx_trim; `roots` names
 * them (the same batch, or one of the same game and size on that context):
 *   osg_ismcts_tree_sizes     host arrays [n]: nodes per root and draws consumed per root (either may be NULL)
 *   osg_ismcts_tree_download  root `root`'s nodes in creation order (node 0 is the root's) into host arrays of `cap`
 *                             rows (>= its node count): player, total_visits, and [cap, 3] by action visits, return_sum
 *                             and expansion rank; `states` (may be NULL; a batch of the same game with >= that many
 *                             rows) receives in row i the state node i was created from, so that
 *                             osg_information_state_string(states, i, player[i]) is the node's key.
 *                             OSG_ERR_UNSUPPORTED when the search had more roots than lanes (a lane's table then holds
 *                             the last of its roots: 512 lanes per compute unit, fewer for large tables); search fewer roots per call. */
typedef struct osg_ismcts_cfg {
  double uct_c;
  int32_t max_simulations;
  int32_t n_rollouts;
  int32_t max_world_samples;       /* <= 0: unlimited */
  int32_t final_policy_type;       /* 1 NORMALIZED_VISITED_COUNT, 2 MAX_VISIT_COUNT, 3 MAX_VALUE */
  int32_t child_selection_policy;  /* 1 UCT, 2 PUCT */
  int32_t max_nodes;
  uint64_t seed;
  int64_t index_offset;
} osg_ismcts_cfg;
int osg_ismcts_search(const osg_batch* roots, const osg_ismcts_cfg* cfg, double* policy, int32_t* sampled_action,
                      int32_t* child_visits, double* child_return_sum, int32_t* expansion_rank, int32_t* nodes,
                      uint8_t* status, int on_host);
int osg_ismcts_tree_sizes(const osg_batch* roots, int32_t* h_nodes, int64_t* h_draws);
int osg_ismcts_tree_download(const osg_batch* roots, int64_t root, int64_t cap, osg_batch* states, int32_t* h_player,
                             int32_t* h_total_visits, int32_t* h_visits, double* h_return_sum, int32_t* h_rank);

/* ---- every reachable position and its game-theoretic value ------------------------------------------------
 * algorithms::GetAllStates (open_spiel/algorithms/get_all_states.h:38-43, get_all_states.cc:28-91;
 * python/algorithms/get_all_states.py:88-142) and algorithms::ValueIteration (open_spiel/algorithms/
 * value_iteration.h:41-42, value_iteration.cc:84-138; python/algorithms/value_iteration.py:73-159) for tic_tac_toe,
 * connect_four (every geometry) and hex without the swap move on boards of up to 64 cells, enumerated level by level
 * (a level = the positions after that many plies) and solved by one backward sweep.  Other games, hex(swap=true),
 * hex(string_rep=explicit) and larger hex boards: OSG_ERR_UNSUPPORTED with a message.
 * Result order: by level, within a level ascending by the canonical key of the position (csrc/osg_solve.h), so the
 * output is unique; position 0 is the initial state.  Arrays over the n positions:
 *   value [n] f64           Returns()[0] at a terminal position, else the max (player 0 to move) / min (player 1) over
 *                           the children; a child that the limits leave out counts 0 (value_iteration.cc:118)
 *   mask [n * mask_words]   the legal actions whose child has the position's value (the layout of osg_legal_mask); zero
 *                           at a terminal position
 *   distance [n] i32        plies to the end under optimal play: 0 at a terminal position, else 1 + that of the child
 *                           chosen among the optimal ones — the nearest end for a win of the mover, the farthest for a
 *                           loss or a draw
 *   edge_off [n + 1] i64, action [edges] i32, child [edges] i64
 *                           the legal actions of position i, ascending, at edge_off[i] .. edge_off[i + 1], and the index
 *                           of each child (-1 where the limits leave it out)
 * osg_solve_create: depth_limit < 0 = none; depth_limit and include_terminals as in get_all_states.cc:36-48 (a terminal
 * position is listed whatever its depth).  max_states <= 0 = 2^26; a game with more positions fails with
 * OSG_ERR_UNSUPPORTED as soon as that is known, and the context stays usable.
 * osg_solve_level_offsets writes levels + 1 host values.  osg_solve_states fills a batch of the same game and of n
 * states with the positions in result order.  osg_solve_lookup: index [query n] i64, the position of each query state
 * in the result or -1, by key and binary search in one launch. */
typedef struct osg_solve osg_solve;
int osg_solve_create(osg_ctx* ctx, const char* game_string, int32_t depth_limit, int32_t include_terminals,
                     int64_t max_states, osg_solve** out);
int osg_solve_destroy(osg_solve* s);
int osg_solve_sizes(const osg_solve* s, int64_t* states, int32_t* levels, int64_t* edges, int64_t* terminals);
int osg_solve_level_offsets(const osg_solve* s, int64_t* h_offsets);
int osg_solve_states(const osg_solve* s, osg_batch* dst);
int osg_solve_values(const osg_solve* s, double* value, int on_host);
int osg_solve_optimal(const osg_solve* s, uint32_t* mask, int32_t* distance, int on_host);
int osg_solve_edges(const osg_solve* s, int64_t* edge_off, int32_t* action, int64_t* child, int on_host);
int osg_solve_lookup(const osg_solve* s, const osg_batch* query, int64_t* index, int on_host);

/* ---- MCTS with the Evaluator outside the kernel (Evaluator interface mcts.h:83-92; the batched shape of
 * alpha_zero_torch/vpevaluator.{h,cc}) ------------------------------------------------------------------
 * Search trees for every root of a batch that persist between calls.  osg_mcts_tree_advance runs every
 * search until it needs its evaluator and reports, per root, in d_request [n] u8:
 *   0 finished (max_simulations run, root proven, or a single root child: mcts.cc:361-366,437-440)
 *   1 wants Prior(state) of the node it is about to expand (mcts.cc:281-283) — only with flag 1;
 *     5 (= 1 | 4) when that node is the search's root (where MCTSBot mixes in Dirichlet noise, mcts.cc:284-292)
 *   2 wants Evaluate(state) of the leaf it has reached (mcts.cc:377-380)
 *   3 paused by max_new_simulations (more simulations to run; nothing wanted)
 * The state a request refers to is written to element i of `leaf` (a batch of the roots' game and size, which
 * also keeps the parked searches' working states: do not modify it between calls).  The next call takes the
 * answers: d_prior [n, num_distinct_actions] f64 (probability of action a at [i, a]; read for roots that
 * reported 1) and d_value [n, num_players] f64 (read for roots that reported 2); either may be NULL when no
 * root reported that request (a root whose answer is missing stays parked and reports its request again).  h_counts (may be NULL) receives the number of roots per request code [4].
 * cfg as for osg_mcts_search (layout ignored: one lane per root; the tree-policy streams are those of layout 1,
 * so with osg_mcts_tree_rollout_values as the evaluator the search is osg_mcts_search's, draw for draw).
 * flags: 1 = priors come from the caller (else uniform over the legal actions, RandomRolloutEvaluator::Prior
 * mcts.cc:74-87; chance nodes always use their ChanceOutcomes()); 2 = dont_return_chance_node (mcts.h:168);
 * 4 = leaves are evaluated inside the launch by RandomRolloutEvaluator(cfg.n_rollouts, cfg.seed) on the streams of
 * osg_mcts_tree_rollout_values: no request 2 is ever reported, and without flag 1 a whole search is one call;
 * 8 (with 1) = every answer to a value request comes WITH the prior of the same state in d_prior (one network forward
 * gives both: alpha_zero_torch/vpevaluator.cc:60-85 caches them per state): the prior is kept until the leaf is
 * expanded on its second visit, so a simulation is ONE evaluator round instead of up to two; a node whose children a
 * garbage collection cleared asks for its prior again (request 1).  d_prior must then be non-NULL in every call. */
typedef struct osg_mcts_tree osg_mcts_tree;
int osg_mcts_tree_create(const osg_batch* roots, const osg_mcts_cfg* cfg, int flags, osg_mcts_tree** out);
int osg_mcts_tree_destroy(osg_mcts_tree* t);
int osg_mcts_tree_advance(osg_mcts_tree* t, osg_batch* leaf, const double* d_prior, const double* d_value,
                          uint8_t* d_request, int max_new_simulations, int64_t* h_counts);
/* The same for a host that holds no device memory: answers and requests in host arrays (staged through buffers
 * the tree owns); values_on_device != 0: the values were left in the tree's own buffer by
 * osg_mcts_tree_rollout_values(t, leaf, NULL). */
int osg_mcts_tree_advance_host(osg_mcts_tree* t, osg_batch* leaf, const double* h_prior, const double* h_value,
                               int values_on_device, uint8_t* h_request, int max_new_simulations, int64_t* h_counts);
/* RandomRolloutEvaluator::Evaluate (mcts.cc:43-72) of every leaf that reported request 2, on the streams
 * of osg_mcts_search: mean Returns() of cfg.n_rollouts playouts into d_value [n, num_players] (device; NULL = the
 * tree's own value buffer, see osg_mcts_tree_advance_host). */
int osg_mcts_tree_rollout_values(osg_mcts_tree* t, const osg_batch* leaf, double* d_value);
/* The outputs of osg_mcts_search (device pointers, any may be NULL) plus child_prior [n, A] f64. */
int osg_mcts_tree_results(osg_mcts_tree* t, int32_t* best_action, int32_t* child_visits, double* child_reward,
                          int8_t* child_outcome, double* child_prior, double* root_stats);
/* One root's whole tree for the host (SearchNode, mcts.h:114-146): osg_mcts_tree_nodes = nodes in use;
 * download fills host arrays of that length: meta (action [0:8) | player + 1 [8:12) | children [12:20) |
 * has outcome [20] | outcome of player 0 + 1 [21:23) | terminal [23]), index of the first child (children are
 * contiguous), explore_count, total_reward, prior. */
/* The actions from root `root` to the node its search is parked at (the state of its pending request), for a
 * host that wants the State with its history.  Returns the length (<= cap) or a negative status. */
int osg_mcts_tree_leaf_path(osg_mcts_tree* t, int64_t root, int32_t* h_actions, int cap);
int64_t osg_mcts_tree_nodes(osg_mcts_tree* t, int64_t root);
int osg_mcts_tree_download(osg_mcts_tree* t, int64_t root, int64_t cap, uint32_t* h_meta, uint32_t* h_first,
                           uint32_t* h_count, double* h_total, double* h_prior);
/* The root node's total_reward / explore_count (alpha_zero.cc:141) into d_value [n] f64 (device); NaN where the root
 * was never visited. */
int osg_mcts_tree_root_values(osg_mcts_tree* t, double* d_value);
/* Dirichlet noise for the roots' priors in one launch (mcts.cc:188-203, 284-292; the arithmetic is dirichlet_row of
 * open_spiel_amd/csrc/osg_selfplay.h).  d_prior [n, A] f64 is mixed IN PLACE at the legal actions of d_mask
 * [n, mask_words] u32 (bit a of word a / 32, as osg_legal_mask writes it): prior = (1 - epsilon) * prior + epsilon *
 * noise, noise = one Gamma(alpha, 1) draw per legal action in ascending order on the stream
 * Rng(seed, index_offset + row, sub), normalised.  Only rows whose d_request byte is 5 are touched (d_request NULL:
 * every row); illegal columns and all other rows are left bit-unchanged.  alpha > 0, 0 <= epsilon <= 1,
 * A <= 32 * mask_words. */
int osg_mcts_root_noise(osg_ctx* ctx, double* d_prior, const uint32_t* d_mask, int mask_words, const uint8_t* d_request,
                        int64_t n, int A, double alpha, double epsilon, uint64_t seed, int64_t index_offset, uint64_t sub);

/* ---- AlphaZero self-play (alpha_zero_torch/alpha_zero.cc PlayGame, python/algorithms/alpha_zero/alpha_zero.py
 * _play_game, replay_buffer.py) -----------------------------------------------------------------------------------
 * The deterministic two-player games: tic_tac_toe, connect_four, hex.  kuhn_poker and leduc_poker answer
 * OSG_ERR_UNSUPPORTED.  The arithmetic is open_spiel_amd/csrc/osg_selfplay.h.
 *
 * osg_replay: a ring of `capacity` training rows that keeps the newest ones.  A row is the game's state record (in
 * an osg_batch of `capacity` states: osg_replay_states lends it, every batch entry point reads it; do not destroy
 * it), policy [A] f32, value f32 (player 0's outcome of the row's game), root_value f32, player i8, action i32.
 * Rows hold states, not observation tensors: pack those for the rows you sample (osg_observation, osg_legal_mask).
 * osg_replay_sizes: rows held, rows ever appended, capacity (synchronises).
 * osg_replay_sample: index[j] = Rng(seed, index_offset + j, 0).below(size) for j < m; state, policy [m, A] and value
 *   [m] of those rows into dst_states (a batch of the game and of m states), d_policy, d_value; d_index [m] i64 (may
 *   be NULL).  An empty ring or m < 1 is OSG_ERR_INVALID.
 * osg_replay_rows: the stored rows d_index [m] i64 names (device; each in [0, capacity)), any output may be NULL. */
typedef struct osg_replay osg_replay;
int osg_replay_create(osg_ctx* ctx, const char* game_string, int64_t capacity, osg_replay** out);
int osg_replay_destroy(osg_replay* buf);
int osg_replay_sizes(osg_replay* buf, int64_t* size, int64_t* total_seen, int64_t* capacity);
osg_batch* osg_replay_states(osg_replay* buf);
int osg_replay_sample(osg_replay* buf, uint64_t seed, int64_t index_offset, int64_t m, osg_batch* dst_states,
                      float* d_policy, float* d_value, int64_t* d_index);
int osg_replay_rows(osg_replay* buf, const int64_t* d_index, int64_t m, float* d_policy, float* d_value,
                    float* d_root_value, int8_t* d_player, int32_t* d_action);

/* osg_selfplay: the environments `envs` play games against themselves, one ply per select + commit, and finished
 * games go to `buf` (both are borrowed and must outlive the object; same game, same context).  Per-environment
 * trajectories of up to max_game_length plies are staged time-major.
 * osg_selfplay_select (one launch): from a search's d_child_visits [n, A] i32, d_best_action [n] i32 and d_root_value
 *   [n] f64 (all device) the policy target p[a] = visits[a] ^ (1 / temperature) / sum and the move: drawn from p on
 *   the stream Rng(seed, index_offset + env, ply_counter[env]) while the environment has played fewer than
 *   temperature_drop moves of its game, d_best_action[env] from then on (no draw).  ply_counter[env] counts the plies the
 *   environment has played since osg_selfplay_create and never resets.  The ply (state record before the move, policy as
 *   f32, action, root value, player) is staged; d_policy_out [n, A] f32 (may be NULL) and d_action_out [n] i32 receive
 *   policy and move.  A row whose visits sum to 0 (or whose state is terminal) is left unrecorded, gets action
 *   OSG_INVALID_ACTION and is counted like an illegal action (osg_ctx_synchronize: OSG_ERR_ILLEGAL).
 * osg_selfplay_commit (four kernels plus a memset and up to two device-to-device copies; no host read-back unless
 *   h_counts is given): applies the chosen moves; a game
 *   ends when its state is terminal, or when |root_value| > cutoff_value, then with returns +-root_value for the mover
 *   (alpha_zero.cc:154-158); the finished trajectories are appended to the ring in ascending environment order, each in
 *   ply order, every row with value = returns[0]; finished environments restart from the initial state.
 *   d_finished [n] u8 and d_returns [n] f64 (player 0's return of a finished game, else 0; either may be NULL);
 *   h_counts [2] (may be NULL): games finished and rows appended by this call.
 * osg_selfplay_staged: ply t of every environment's running trajectory (any output may be NULL; dst_states: a batch
 *   of the game and of n states), d_length [n] i32 the plies staged per environment, d_ply_counter [n] i64. */
typedef struct {
  double temperature;        /* finite and > 0 */
  double cutoff_value;       /* > max_utility: never */
  int32_t temperature_drop;
  int32_t reserved;
  uint64_t seed;
  int64_t index_offset;
} osg_selfplay_cfg;
typedef struct osg_selfplay osg_selfplay;
int osg_selfplay_create(osg_batch* envs, osg_replay* buf, const osg_selfplay_cfg* cfg, osg_selfplay** out);
int osg_selfplay_destroy(osg_selfplay* sp);
int osg_selfplay_select(osg_selfplay* sp, const int32_t* d_child_visits, const int32_t* d_best_action,
                        const double* d_root_value, float* d_policy_out, int32_t* d_action_out);
int osg_selfplay_commit(osg_selfplay* sp, uint8_t* d_finished, double* d_returns, int64_t* h_counts);
int osg_selfplay_staged(osg_selfplay* sp, int t, osg_batch* dst_states, float* d_policy, int32_t* d_action,
                        float* d_root_value, int8_t* d_player, int32_t* d_length, int64_t* d_ply_counter);

/* ---- tabular CFR family -------------------------------------------------- */
/* osg_cfr_cfg.kernel (the field's comment below says what each one forces) */
#define OSG_CFR_KERNEL_AUTO 0
#define OSG_CFR_KERNEL_GENERAL 1
#define OSG_CFR_KERNEL_GRID 2
#define OSG_CFR_KERNEL_PATH 3
#define OSG_CFR_KERNEL_SPLIT 4
#define OSG_CFR_KERNEL_SUB 5
typedef struct {
  int32_t alternating_updates;   /* CFRSolverBase ctor (cfr.h:190-196)            */
  int32_t linear_averaging;
  int32_t regret_matching_plus;
  int32_t solver;                /* 0: CFRSolverBase family, tables start at 0 (cfr.h:47-52);
                                    1: ExternalSamplingMCCFRSolver, regrets and cumulative policy
                                       start at kInitialTableValues = 1e-6
                                       (external_sampling_mccfr.h:59, .cc:142-143);
                                    2: OutcomeSamplingMCCFRSolver (outcome_sampling_mccfr.cc:141-241,
                                       Baseline() == 0), same initial values, same mini-batch
                                       protocol through osg_mccfr_sample / osg_mccfr_iterate        */
  double epsilon;                /* solver 2 only: OutcomeSamplingMCCFRSolver's exploration
                                    (outcome_sampling_mccfr.h:43 kDefaultEpsilon = 0.6)          */
  int32_t kernel;                /* OSG_CFR_KERNEL_*: AUTO; GENERAL forces the general level-synchronous
                                    kernel (k_cfr) even where the all-in-LDS small-tree kernel applies;
                                    GRID forces the full-grid phase kernels (auto for trees > 65536
                                    histories); PATH forces the single-workgroup path kernel; SPLIT =
                                    auto's choice for trees that start with their chance deals and
                                    split into <= #CUs subtrees of <= 1024 histories (leduc_poker): one
                                    workgroup per deal subtree, one grid barrier per player pass; SUB =
                                    auto's choice for the big trees of that shape (3-player
                                    leduc_poker: 1.8 M histories): ONE cooperative launch, a workgroup
                                    per deal subtree of up to 8192 histories, two grid barriers per
                                    player pass (alternating updates only)                        */
  int32_t replicas;              /* 0 or 1: one solver.  B > 1: B independent solvers of the same
                                    game advanced together, one workgroup each (CFR family, trees
                                    that fit LDS); select one with osg_cfr_select_replica         */
  int32_t random_initial_regrets;/* CFRSolverBase ctor (cfr.h:190-196): regrets start at
                                    0.001 * U[0,1) (cfr.cc:31,249-252) from the counter stream
                                    (seed, replica_offset + replica, infostate, action)           */
  uint64_t seed;
  int64_t replica_offset;        /* global index of replica 0 (sharding replicas over GPUs)       */
} osg_cfr_cfg;
/* Replaces CFRSolverBase::CFRSolverBase + InitializeInfostateNodes
 * (cfr.cc:191-261): expands the whole game tree level by level ON THE DEVICE
 * (legal-mask / apply / status kernels), numbers infostates, uploads the
 * level-ordered arrays and zero-initialised [I, Amax] fp64 tables. */
int osg_cfr_create(osg_ctx* ctx, const char* game_string, const osg_cfr_cfg* cfg, osg_cfr** out);
int osg_cfr_destroy(osg_cfr* s);
/* out[0..5] = histories, chance nodes, decision nodes, terminal nodes, infostates, Amax */
int osg_cfr_sizes(const osg_cfr* s, int64_t* out);
/* Back to iteration 0 with freshly initialised tables. */
int osg_cfr_reset(osg_cfr* s);
/* CFRSolverBase::EvaluateAndUpdatePolicy x iters (cfr.cc:263-282): one launch, all iterations. */
int osg_cfr_iterate(osg_cfr* s, int iters);
/* Number of EvaluateAndUpdatePolicy calls (or MCCFR mini-batches) done so far. */
int osg_cfr_iteration(const osg_cfr* s);
/* Diagnostic: the kernel family the solver's last iterate / sample call launched ("k_cfr_small<lds, owner>", "k_cfr_split",
 * "k_mccfr_resident_flat", "k_mccfr_resident<split 2>", ...; "" before the first launch or for the remaining forms).  The
 * parity tests and bench.py record it next to what they checked (no reference counterpart). */
const char* osg_cfr_last_kernel(const osg_cfr* s);
/* Diagnostic: the form the last policy evaluation took ("k_geval": a launch per level and phase, "k_geval_persist": one
 * persistent launch — opt-in, OSG_EVAL_PERSIST=1 —, "k_eval_jobs", "k_policy_eval"; "" before the first).  No reference counterpart. */
const char* osg_cfr_last_eval_kernel(const osg_cfr* s);
/* Number of replicas, and which one the table accessors / osg_cfr_evaluate_policy / upload act on. */
int osg_cfr_replicas(const osg_cfr* s);
int osg_cfr_select_replica(osg_cfr* s, int replica);
/* Restores the iteration counter of a deserialised solver (cfr.h:318-323 deserialisation ctor). */
int osg_cfr_set_iteration(osg_cfr* s, int iteration);
/* Discounted CFR (Brown & Sandholm 2019; discounted_cfr.py:93-209, DCFRSolver(alpha = 3/2, beta = 0, gamma = 2), LCFRSolver =
 * (1, 1, 1)) for the osg_cfr_iterate calls that follow: in iteration t, after player p's pass, every cumulative regret of
 * p's infostates is multiplied by t^alpha / (t^alpha + 1) if it is >= 0 and by t^beta / (t^beta + 1) otherwise, and with
 * linear_averaging the cumulative-policy term is reach * prob * t^gamma.  enabled = 0 turns it off again.  OSG_ERR_INVALID
 * for enabling it on an MCCFR solver, with regret_matching_plus or with simultaneous updates, and for a negative or
 * non-finite exponent whatever `enabled` says; osg_cfr_br_iterate
 * refuses a discounting solver.  osg_cfr_reset keeps the setting; a checkpoint is restored by osg_cfr_create,
 * osg_cfr_set_discounting, osg_cfr_upload_tables, osg_cfr_set_iteration.  osg_cfr_last_kernel carries a `dcfr` tag. */
int osg_cfr_set_discounting(osg_cfr* s, int enabled, double alpha, double beta, double gamma);
/* The three factors of iteration t >= 1 exactly as the kernels use them (formed on the host in double precision with
 * std::pow, handed to a launch as a table): out = {t^alpha / (t^alpha + 1), t^beta / (t^beta + 1), t^gamma}.  Needs no device. */
int osg_cfr_discount_factors(double alpha, double beta, double gamma, int iteration, double out[3]);
/* ExternalSamplingMCCFRSolver::FullUpdateAverage (external_sampling_mccfr.cc:188-231) — AverageType::kFull:
 * one full-tree pass adding weight * reach_probs[cur_player] * sigma(I)[a] to the cumulative policy of every
 * decision history, sigma = regret matching of the regrets as they are now.  weight = 1 after each
 * RunIteration's traversals is the reference; a mini-batch of T trajectories stands for T / P iterations. */
int osg_mccfr_full_average(osg_cfr* s, double weight);

/* AverageType of an external-sampling solver (external_sampling_mccfr.h:48): 0 kSimple (default), 1 kFull —
 * the traversals' sampled average-policy terms are dropped and osg_mccfr_iterate ends with
 * osg_mccfr_full_average(trajectories / P) when the batch holds at least one whole iteration. */
int osg_mccfr_set_average_type(osg_cfr* s, int average_type);

/* ONE UpdateRegrets(root, player, rng) (external_sampling_mccfr.cc:122-186) whose uniforms are
 * h_uniforms[0], h_uniforms[1], ... in visiting order instead of the counter stream — with the doubles
 * std::uniform_real_distribution<double>(0, 1) draws from the caller's std::mt19937 this IS the reference's
 * traversal, draw for draw (RunIteration(std::mt19937*), external_sampling_mccfr.h:63-100).  Fills the
 * delta tables like osg_mccfr_sample (fold with osg_mccfr_apply_deltas); *consumed = uniforms used. */
int osg_mccfr_sample_uniforms(osg_cfr* s, int player, const double* h_uniforms, int n, int32_t* consumed);

/* CFRBRSolver::EvaluateAndUpdatePolicy (cfr_br.cc:48-83) x iters on a CFRSolverBase table (solver 0,
 * no linear averaging, no RM+): every player's best response to the current policy
 * (TabularBestResponse, best_response.cc:194-227), one regret / average-policy pass per player with
 * the other players following their best responses, ApplyRegretMatching. */
int osg_cfr_br_iterate(osg_cfr* s, int iters);

/* Extensive-form fictitious play: XFPSolver.iteration() (open_spiel/python/algorithms/fictitious_play.py:165-240; Heinrich,
 * Lanctot and Silver 2015, Algorithm 1) x iters on a CFRSolverBase object (solver 0, one replica, no discounting).  The
 * AVERAGE policy lives in the current-policy table, uniform after osg_cfr_create / osg_cfr_reset; the regret and
 * cumulative-policy tables are not touched, and a later osg_cfr_iterate overwrites the current-policy table.  One
 * iteration: every player's best response to the average policy (TabularBestResponse, best_response.cc:194-227: the first
 * legal action with the maximal counterfactual-weighted value; the first legal action where there is no counterfactual
 * reach), then at every infostate of player p, with alpha = 1 / (iterations + 1) formed on the host in double precision
 * after the counter was raised (fictitious_play.py:166,228), avg_reach / br_reach the products of p's own action
 * probabilities on the way there under the average policy / the best response (1.0 at the root, multiplied root to leaf,
 * all taken from the table as it was before the iteration),
 *   new[a] = avg[a] + (alpha * br_reach * (br[a] - avg[a])) / ((1.0 - alpha) * avg_reach + alpha * br_reach)
 * in exactly that order (fictitious_play.py:232-236), not contracted.  osg_cfr_iteration counts the iterations.  A
 * checkpoint is restored with osg_cfr_upload_tables(cur_policy) and osg_cfr_set_iteration; an uploaded policy with zero
 * probabilities gives the reference's IEEE result where both reaches vanish (0 / 0 = NaN), not an error.
 * OSG_ERR_INVALID for an MCCFR solver and for a discounting solver, OSG_ERR_UNSUPPORTED for replicas > 1 and for a tree
 * with an information state that spans several levels; the message names the reason.
 * osg_cfr_last_kernel afterwards: "k_xfp_small" — ONE launch of one workgroup for all iterations, the policy and the best
 * response's scratch in LDS (trees one workgroup evaluates: the kuhn_poker family) —, or the general form, a best-response
 * evaluation and two launches (reach, update) per iteration, named after the evaluation it used: "k_xfp<k_policy_eval>",
 * "k_xfp<k_eval_jobs>" (leduc_poker), "k_xfp<k_geval>" (3-player leduc_poker; osg_cfr_cfg.kernel = 2 forces it).
 * osg_cfr_cfg.kernel = 1 forces the general form with the one-workgroup evaluation.  Both forms give the same bits. */
int osg_xfp_iterate(osg_cfr* s, int iters);
/* The averaging half of one iteration (fictitious_play.py:184-240) with the CALLER's best responses: h_best_index [I], an
 * index among each row's legal actions as osg_cfr_best_response returns it.  Raises the iteration counter.  This is where
 * approximate or learned best responses enter (fictitious self-play).  OSG_ERR_INVALID for an index out of range: the
 * table and the counter are left as they were.  osg_cfr_last_kernel: "k_xfp_update". */
int osg_xfp_update(osg_cfr* s, const int32_t* h_best_index);
/* Diagnostic: the two [I] vectors avg_reach and br_reach the next update would use, for h_best_index as above or, where it
 * is NULL, for the device's own best responses to the current-policy table.  Changes neither table nor counter. */
int osg_xfp_reaches(osg_cfr* s, const int32_t* h_best_index, double* h_avg_reach, double* h_br_reach);

/* Magnetic mirror descent over the sequence form with dilated entropy: MMDDilatedEnt
 * (open_spiel/python/algorithms/mmd_dilated.py:132-366 with sequence_form_utils.py:120-228,325-389; Sokota et al. 2023,
 * arXiv 2206.05825) on a CFRSolverBase object (solver 0, no discounting) of a two-player zero-sum game.  The behavioural
 * policy pi lives in the current-policy table and the average sequences avg_x in the cumulative-policy table, so
 * osg_cfr_tables(avg_policy) and osg_cfr_evaluate_policy(which = 0) give the average policy (sequence_to_policy,
 * sequence_form_utils.py:284-322) and which = 1 the last iterate; the regret table is not touched.  With alpha > 0 the last
 * iterate converges linearly to the alpha-reduced normal-form QRE, with alpha = 0 the average converges to a Nash
 * equilibrium.  csrc/osg_mmd.h has the arithmetic of one update_sequences() (mmd_dilated.py:261-323) and its fixed
 * orders of summation; no floating-point atomics, two runs and both kernel forms give the same bits.
 *
 * osg_mmd_default_stepsize: alpha / max|payoff_mat|^2 (mmd_dilated.py:169), the matrix formed on the host once per solver
 * (sequence_form_utils.py:148-153,207-228). */
int osg_mmd_default_stepsize(osg_cfr* s, double alpha, double* out);
/* alpha[n], stepsize[n]: one pair per replica (n = osg_cfr_replicas).  The first accepted call puts the solver into
 * mirror-descent mode (mmd_dilated.py:174-176): avg_x = x of the current-policy table (uniform on a fresh solver), counter 0.
 * Later calls change the parameters only, so an annealing schedule keeps the state (the reference's `alpha` and `stepsize`
 * attributes).  OSG_ERR_INVALID for an MCCFR or a discounting solver, n != replicas, and a negative or non-finite alpha or
 * stepsize (mmd_dilated.py:149); OSG_ERR_UNSUPPORTED for a game with other than two players (mmd_dilated.py:142), an
 * information state that spans several tree levels, and replicas > 1 where only the general form serves the solver.  A
 * refused call changes nothing.  In mirror-descent mode osg_cfr_iterate, osg_cfr_br_iterate and osg_xfp_iterate answer
 * OSG_ERR_INVALID; osg_cfr_reset returns to the uniform start (avg_x = x, counter 0) and keeps the parameters. */
int osg_mmd_set_params(osg_cfr* s, int n, const double* alpha, const double* stepsize);
/* update_sequences() x iters (mmd_dilated.py:261-281) for every replica, each with its own pair.  osg_cfr_iteration counts
 * the calls (the reference's iteration_count - 1).  A checkpoint is osg_cfr_upload_tables(cum_policy = avg_x, cur_policy =
 * pi) and osg_cfr_set_iteration.  OSG_ERR_INVALID before osg_mmd_set_params.  osg_cfr_last_kernel afterwards:
 * "k_mmd_small" — ONE launch for all iterations, a workgroup per replica with pi, x, avg_x in LDS (tables up to 128 KiB:
 * the kuhn_poker family, leduc_poker) —, or "k_mmd", a launch per infostate level and one for the average per iteration
 * (osg_cfr_cfg.kernel = 1 forces it; one replica). */
int osg_mmd_iterate(osg_cfr* s, int iters);
/* get_gap() (mmd_dilated.py:325-359) of the selected replica's policy at its alpha: the saddle-point gap of the
 * regularised game.  OSG_ERR_INVALID where that alpha is 0 (mmd_dilated.py:333).  Changes neither table nor counter. */
int osg_mmd_gap(osg_cfr* s, double* out);
/* current_sequences() (which = 0, mmd_dilated.py:368-374: x of the current-policy table) or get_avg_sequences() (which = 1,
 * :376-382) of the selected replica as an [I, Amax] host array, cell (I, a) the sequence value, padding 0. */
int osg_mmd_sequences(osg_cfr* s, int which, double* h_x);

/* Extensive-form regret minimization: EFRSolver (open_spiel/python/algorithms/efr.py; Morrill et al. 2021, arXiv 2102.06973)
 * on a CFRSolverBase object (solver 0, no discounting, one replica) of kuhn_poker or leduc_poker with any served number of
 * players.  The current policy lives in the current-policy table and the reach-weighted cumulative policy in the
 * cumulative-policy table, so osg_cfr_tables, osg_cfr_evaluate_policy and osg_cfr_action_values read them as they read
 * CFR's; the regret table is not touched: EFR's regrets are per (information state, deviation).  One iteration updates
 * all players at once, with no alternation and no linear averaging (efr.py:424-433).  csrc/osg_efr.h has the arithmetic,
 * the reference's behaviour it restates and its fixed orders of summation; no floating-point atomics, two runs and both
 * kernel forms give the same bits.
 *
 * osg_efr_set_deviations: builds the deviation tables of set `type` on the host from the solver's tree and starts from the
 * uniform policy with R = 0, counter 0.  type: 0 blind action, 1 informed action, 2 blind cf, 3 informed cf, 4 bps,
 * 5 cfps, 6 csps, 7 tips, 8 bhv (efr.py:465-488).  form: 0 by tree size (<= 4096 histories: resident), 1 "k_efr_resident"
 * — ONE launch of one workgroup runs all iterations of a call —, 2 "k_efr" — a launch per phase, tree level and
 * own-decision depth.  OSG_ERR_INVALID for an MCCFR, discounting or mirror-descent solver, an unknown type or form;
 * OSG_ERR_UNSUPPORTED for replicas > 1, a policy row wider than 4 actions, more than 8 earlier own decisions on a path,
 * more than 2^26 deviations.  Afterwards osg_cfr_iterate answers OSG_ERR_INVALID and osg_cfr_reset returns to the start. */
int osg_efr_set_deviations(osg_cfr* s, int type, int form);
/* evaluate_and_update_policy() x iters (efr.py:424-433).  OSG_ERR_INVALID before osg_efr_set_deviations. */
int osg_efr_iterate(osg_cfr* s, int iters);
/* out[5]: deviations in total, the most of one information state, L (the most earlier own decisions on a path, at least
 * 1), the doubles of the regret state (osg_efr_regrets), own-decision depths. */
int osg_efr_sizes(const osg_cfr* s, int64_t* out);
/* The tables, for tests; any pointer may be NULL.  dev_off [I + 1]: the deviations of information state i are
 * dev_off[i] .. dev_off[i + 1], in the reference's order.  Per deviation: target and source (-1: external) as indices among
 * the row's legal actions; weights_none (1: the reference's `None` weight vector); weights [D, L] (0 / 1, -1 padding and
 * with weights_none) and memory [D, L] (remembered action ids, -1 padding) as the reference states them; y_slot (the index
 * of its swap among the information state's distinct swaps, in order of first appearance); cells [D, L]: for every
 * remembered decision the cell (earlier information state * Amax + column) of the current-policy table whose product is
 * memreach, -2 where the reference reads a probability that is always 0, -1 where nothing is remembered. */
int osg_efr_deviations(const osg_cfr* s, int32_t* dev_off, int8_t* target, int8_t* source, int8_t* weights_none, int8_t* weights,
                       int8_t* memory, int32_t* y_slot, int32_t* cells);
/* The regret state as osg_efr_sizes out[3] doubles: R per deviation, then the y values [I, 16] an information state
 * carries into the next policy pass when the regret pass reaches none of its histories (efr.py:338,351).  A checkpoint is
 * this, the cumulative and current policy tables (osg_cfr_upload_tables) and the counter (osg_cfr_set_iteration). */
int osg_efr_regrets(osg_cfr* s, double* h_state);
int osg_efr_upload_regrets(osg_cfr* s, const double* h_state);

/* ExternalSamplingMCCFRSolver::RunIteration (external_sampling_mccfr.cc:71-186,
 * AverageType::kSimple) for `trajectories` traverser passes (player = global
 * trajectory index mod P), mini-batched: every trajectory of one call reads the
 * tables as they were at the start of the call and adds its deltas atomically.
 * Tables start at kInitialTableValues = 1e-6 (external_sampling_mccfr.h:59). */
int osg_mccfr_iterate(osg_cfr* s, uint64_t seed, int64_t first_trajectory, int64_t trajectories);
/* The sampling half of osg_mccfr_iterate: zero the delta tables, run the traversals,
 * leave the regret / average-policy deltas in the delta tables (osg_mccfr_delta_ptrs)
 * WITHOUT folding them in.  Trajectory g (global index) draws from the counter stream
 * (seed, g) and updates player g mod P, so a batch can be split across GPUs by index.
 * External sampling: the draws below the traverser's first two nodes come from sub-streams
 * of (seed, g) — one per child subtree, in visiting order inside it — so that small
 * mini-batches can walk those subtrees on separate lanes (same sums as on one lane;
 * csrc/osg_cfr.hip es_stream, restated by the oracle's replay).  osg_mccfr_apply_deltas
 * leaves the delta tables zero. */
int osg_mccfr_sample(osg_cfr* s, uint64_t seed, int64_t first_trajectory, int64_t trajectories);
/* Device pointers to the [I, Amax] fp64 tables: regrets, cumulative policy,
 * current policy (for RCCL all-reduce by the caller, or inspection). */
int osg_cfr_table_ptrs(osg_cfr* s, double** d_regrets, double** d_cum_policy, double** d_cur_policy);
/* MCCFR mini-batch protocol for multi-GPU: deltas accumulate into separate
 * [I, Amax] buffers; the caller all-reduces them (RCCL) and then folds them in.
 * CONTRACT for the solver's own delta buffers (these and osg_mccfr_spare_delta_buffer's): the caller may write them
 * only between a sample and the apply that follows it (the in-place all-reduce does exactly that).  osg_mccfr_apply_deltas
 * leaves a buffer zero and the next osg_mccfr_sample relies on it — it skips its fill launch for a buffer the last fold
 * left clean — so anything written into the buffer after the apply is added to the next mini-batch.  Caller-owned
 * buffers (osg_mccfr_sample_into with memory of the caller) are always zero-filled first. */
int osg_mccfr_delta_ptrs(osg_cfr* s, double** d_regret_delta, double** d_policy_delta);
int osg_mccfr_apply_deltas(osg_cfr* s);
/* The same two halves on a CALLER's delta buffer d_delta = regret deltas [I, Amax] | average-policy deltas
 * [I, Amax] (2 * I * Amax device doubles, 8-byte aligned; NULL = the solver's own tables): with two such
 * buffers a host overlaps the all-reduce of mini-batch k with the traversals of mini-batch k + 1, which then
 * read the tables without k's deltas (stale by one mini-batch; ShardedMccfr(overlap=True) in
 * open_spiel_amd/distributed.py, ExternalSamplingMCCFRSolver::RunShardedMiniBatch(..., overlap) in the host
 * mirror).  The reference has no such schedule: its RunIteration is sequential (external_sampling_mccfr.cc:71-80). */
int osg_mccfr_sample_into(osg_cfr* s, uint64_t seed, int64_t first_trajectory, int64_t trajectories, double* d_delta);
int osg_mccfr_apply_deltas_from(osg_cfr* s, double* d_delta);
/* Two such buffers owned by the solver (allocated on first request, freed with it) for hosts that have no
 * device allocator of their own (which = 0 | 1). */
int osg_mccfr_spare_delta_buffer(osg_cfr* s, int which, double** d_delta);
/* Overwrite the [I, Amax] tables from host arrays (any may be NULL): restores a
 * checkpoint / CFRInfoStateValuesTable (cfr.cc:723-777 deserialisation target). */
int osg_cfr_upload_tables(osg_cfr* s, const double* h_regrets, const double* h_cum_policy,
                          const double* h_cur_policy);
/* CFRInfoStateValuesTable rows (cfr.h:42-104) to the host: arrays [I, Amax] (padding 0),
 * nact[I], legal[I, Amax] (padding -1), avg_policy per cfr.cc:104-125. Any may be NULL. */
int osg_cfr_tables(const osg_cfr* s, int32_t* nact, int32_t* legal, double* regrets,
                   double* cum_policy, double* cur_policy, double* avg_policy);
/* Policy evaluation on the flattened tree: algorithms::ExpectedReturns (expected_returns.cc:34-130),
 * TabularBestResponse values for every player (best_response.cc:194-227), NashConv and
 * Exploitability (tabular_exploitability.cc:30-89).  which_policy: 0 the tables' average policy
 * (cfr.cc:104-125), 1 their current policy, 2 the [I, Amax] host table h_policy (rows in the
 * solver's infostate order, osg_cfr_infostate_key).  expected_returns / best_response_values are
 * [P]; any output may be NULL. */
int osg_cfr_evaluate_policy(osg_cfr* s, int which_policy, const double* h_policy, double* expected_returns,
                            double* best_response_values, double* nash_conv, double* exploitability);

/* TabularBestResponse (best_response.h:38-130, best_response.cc:194-227) against the same policy choices as
 * osg_cfr_evaluate_policy: h_best_index [I] receives, for every infostate (of every player: each player responds
 * to the others playing the policy), the index among its legal actions of the best-response action (ties and
 * unreachable infostates: the first); best_response_values [P] (may be NULL) the responders' values. */
int osg_cfr_best_response(osg_cfr* s, int which_policy, const double* h_policy, int32_t* h_best_index,
                          double* best_response_values);
/* TabularBestResponse::Value(history) (best_response.h:127-128, best_response.cc:229-262) for EVERY history of the
 * flattened tree at once: h_history_values [H] (osg_cfr_sizes[0]) receives the value for `responder` of each history
 * when it best-responds from there on and the others follow the policy (choices as for osg_cfr_evaluate_policy). */
int osg_cfr_best_response_history_values(osg_cfr* s, int which_policy, const double* h_policy, int responder,
                                         double* h_history_values);
/* Per-infostate action values and reaches of a policy profile: TreeWalkCalculator (open_spiel/python/algorithms/
 * action_value.py:87-216) and, with a best responder, Calculator (action_value_vs_best_response.py:63-156).  Every
 * player plays the policy which_policy selects (as for osg_cfr_evaluate_policy; 2: the [I, Amax] table `policy`), except
 * `responder` (-1: nobody; two-player games only, action_value_vs_best_response.py:67), who plays the deterministic
 * TabularBestResponse to it exactly as osg_cfr_best_response picks it.  For a member history h of infostate i (player
 * p): r_q(h) the product of player q's probabilities on the root path, c(h) chance's, reach(h) = r_0 * ... * c,
 * opp(h) = prod_{q != p} r_q, v(h) the profile's expected returns below h.  Summed over an infostate's member histories
 * in the reference's visiting order:
 *   reach = sum reach(h) (info_state_prob), cf_reach = sum c(h) * opp(h) (counterfactual_reach_probs), chance_reach =
 *   sum c(h) (info_state_chance_prob), player_reach = r_p(h) of a member (player_reach_probs),
 *   weighted_values[i, a, q] = sum v_q(child(h, a)) * reach(h) (weighted_action_values, :148),
 *   action_values[i, a] = weighted_values[i, a, p] / reach[i] where reach[i] > 0, else 0 (:202-204),
 *   cf_reach_by_value[i, a] = sum (v_p(child(h, a)) * opp(h)) * c(h) (sum_cfr_reach_by_action_value, :149-151),
 *   root_values = v(root) (root_node_values); best_response_value = the responder's best-response value (Calculator's
 *   `exploitability`), best_index its choice at its rows (an index among the row's legal actions), -1 elsewhere.
 * Rows in the solver's infostate order, columns the row's legal actions ascending, padding cells 0.  on_host = 1:
 * `policy` and the outputs are host memory and the call returns when they have arrived; on_host = 0: they are device
 * memory and everything is enqueued on the context's stream (but for the best-response evaluation of a responder, which
 * waits as osg_cfr_best_response does).  A refused call writes nothing.  The sums have one fixed order (no atomics):
 * two calls give the same bits, in either kernel form (osg_cfr_cfg.kernel = 2 forces the launch-per-level form;
 * osg_cfr_last_eval_kernel names the one taken). */
typedef struct {
  double* root_values;         /* [P] */
  double* action_values;       /* [I, Amax] */
  double* cf_reach;            /* [I] */
  double* player_reach;        /* [I] */
  double* reach;               /* [I] */
  double* chance_reach;        /* [I] */
  double* cf_reach_by_value;   /* [I, Amax] */
  double* weighted_values;     /* [I, Amax, P] */
  double* best_response_value; /* [1], responder >= 0 only */
  int32_t* best_index;         /* [I], responder >= 0 only */
} osg_action_values_out;       /* any member may be NULL */
int osg_cfr_action_values(osg_cfr* s, int which_policy, const double* policy, int responder, int on_host,
                          const osg_action_values_out* out);
/* Populations of policies (PSRO / double oracle, open_spiel/python/algorithms/psro_v2/): `tables` is a stack
 * [n_tables, I, Amax] of policy tables in the layout which_policy = 2 uses (rows in the solver's infostate order, columns
 * the row's legal actions ascending, padding cells ignored); "policy k of player p" is table k's rows at p's infostates.
 * A solver created in any mode may be used: its own tables are neither read nor written.  The games have perfect recall.
 *
 * osg_cfr_profile_returns: the payoff-tensor cells expected_game_score.policy_value
 * (open_spiel/python/algorithms/expected_game_score.py:35-58) gives one tree walk at a time.  profiles is [n_profiles, P]
 * int32: in profile m player q follows table profiles[m, q], and returns[m, :] = policy_value(root, [policy_{profiles[m, 0]}
 * .. policy_{profiles[m, P-1]}]).  The whole tensor is the call with the cartesian product, PSRO's update the call with
 * the new cells.  Computed in sequence form: returns[m, q] = sum over the terminals z of u_q(z) * c(z) * prod_p
 * plan_{profiles[m, p]}(p's last action before z), plan_k[i, a] = (player's own reach of i under table k) * table k[i, a];
 * csrc/osg_population.h has the arithmetic and the one order of the sum.  The bits of returns[m, :] depend on the game and
 * on the P tables profile m names, not on its position, on n_profiles, on the other profiles or tables or on on_host.
 *
 * osg_cfr_aggregate_policies: PolicyAggregator.aggregate (open_spiel/python/algorithms/policy_aggregator.py:130-265) for
 * all players at once: the behavioural policy that is realization-equivalent to every player p mixing its tables with
 * weights[p, :] ([P, n_tables]).  For infostate i of player p and legal action a, over i's member histories h in the
 * reference's visiting order and k ascending, acc[i, a] += reach_k(h) * table k[i, a], reach_k(h) = weights[p, k] times
 * p's own probabilities under table k on h's root path in path order; out[i, a] = (acc[i, a] + epsilon) / sum_a'
 * (acc[i, a'] + epsilon) (:171-178; the reference's epsilon is 1e-40), padding cells 0.  A table of weight 0 contributes
 * nothing; a row no table reaches comes out uniform.
 *
 * on_host = 1: every pointer is host memory and the call returns when the outputs have arrived.  on_host = 0: every
 * pointer is device memory and everything is enqueued on the context's stream without waiting (the first population call
 * on a solver also builds and uploads the terminals' plan indices, which waits).  A refused call writes nothing and sets
 * osg_last_error: a null pointer, n_tables < 1, a profile index outside [0, n_tables), a negative or non-finite weight,
 * epsilon < 0 (OSG_ERR_INVALID); more than 2^22 profiles per call, a table stack of more than 2^30 bytes (n_tables * I *
 * Amax * 8; the solver keeps as much scratch again, and on_host = 1 a device copy of the stack), rows wider than 8 actions
 * (OSG_ERR_UNSUPPORTED, the message names the limit).  With on_host = 0 the indices and weights are checked on the
 * device: the refused call's kernels write nothing, and the next population call on the solver returns the error instead
 * of running.  osg_cfr_last_eval_kernel: "k_pop_returns", "k_pop_aggregate" (one form each). */
int osg_cfr_profile_returns(osg_cfr* s, const double* tables, int n_tables, const int32_t* profiles, int64_t n_profiles,
                            int on_host, double* returns /* [n_profiles, P] */);
int osg_cfr_aggregate_policies(osg_cfr* s, const double* tables, int n_tables, const double* weights /* [P, n_tables] */,
                               double epsilon, int on_host, double* out_table /* [I, Amax] */);
/* The flattened tree's edges: parent [H] (-1 at the root) and the action / chance outcome on the edge from the
 * parent [H] (-1 at the root); histories are numbered level by level.  Either may be NULL. */
int osg_cfr_tree_edges(const osg_cfr* s, int32_t* parent, int32_t* action);
/* InformationStateString() of infostate i (kuhn_poker.cc:109-166, leduc_poker.cc:198-239).
 * Returns the length (excluding NUL), or <0. */
int osg_cfr_infostate_key(const osg_cfr* s, int64_t i, char* buf, int cap);
/* The player who acts at infostate i (State::CurrentPlayer() of its histories), -1 for a bad index. */
int osg_cfr_infostate_player(const osg_cfr* s, int64_t i);

/* ---- PSRO's meta-strategy solvers on a batch of normal-form meta-games --------------------------
 * Projected replicator dynamics (open_spiel/python/algorithms/projected_replicator_dynamics.py) and regret matching
 * (regret_matching.py) with nfg_utils.StrategyAverager's average: psro_v2's "prd" and "rm".  A problem is P payoff
 * tensors [K_0 .. K_{P-1}], one per player, row-major; a call holds n_problems of one shape and runs every iteration of
 * every problem in ONE launch, a workgroup per problem, with the strategies, regrets and sums in LDS and registers.
 * csrc/osg_meta_solver.h has the arithmetic and the one order of every sum; the reference's sums go through BLAS, so it is
 * matched within rounding, not bit for bit.  The bits of a problem's result depend on its tensors, its cfg and its initial
 * strategies, not on its position, on n_problems, on the other problems, on `form` or on on_host.
 *   cfgs      n_cfgs = 1: one cfg for every problem; n_cfgs = n_problems: problem b runs cfgs[b] (a sweep of dt, gamma,
 *             iterations or method over copies of one meta-game, or many meta-games, is one launch).  ALWAYS host memory.
 *   form      0: the tensors are staged in LDS where P * K_0 * .. * K_{P-1} doubles fit the workgroup's LDS limit (from
 *             the device's properties) beside the strategies, and read from global memory otherwise; 1 / 2 name one
 *             (1 where it does not fit: OSG_ERR_UNSUPPORTED).  Every cfg of a call names the same form.
 *   window    0: the average of the whole trajectory (the initial strategies and every iteration); n > 0: of the last
 *             min(n, iterations + 1) entries (average_over_last_n_strategies).
 *   initial   [n_problems, sum K_p], player after player, or NULL: uniform.  iterations = 0 returns it.
 *   average, last   [n_problems, sum K_p]: the averaged strategies and the last iterate; last may be NULL.
 * on_host = 1: tensors, initial, average and last are host memory and the call returns when the outputs have arrived;
 * on_host = 0: they are device memory and the launch is enqueued on the context's stream.
 * A refused call writes nothing.  OSG_ERR_INVALID: a null ctx, shape, cfgs, tensors or average, n_problems < 0, n_cfgs
 * neither 1 nor n_problems, a method other than 0 / 1, iterations or window < 0, a form outside 0..2 or not the same in
 * every cfg, a dt or gamma that is not finite.  OSG_ERR_UNSUPPORTED: fewer than 2 or more than 5 players, a K_p outside
 * 1..64, more than 2^22 cells per tensor, more than 10^8 iterations, more than 2^20 problems or 2^32 bytes of tensors per
 * call.  The tensors are expected finite. */
typedef struct osg_meta_cfg {
  int32_t method;       /* 0 projected replicator dynamics, 1 regret matching */
  int32_t iterations;
  double dt;            /* projected replicator dynamics only (prd_dt) */
  double gamma;         /* prd_gamma / gamma */
  int32_t window;       /* 0: the whole trajectory */
  int32_t use_approx;   /* projected replicator dynamics only: _approx_simplex_projection */
  int32_t form;         /* 0 by size, 1 tensors resident in LDS, 2 tensors read from global memory */
  int32_t reserved;     /* 0 */
} osg_meta_cfg;
int osg_meta_solve(osg_ctx* ctx, int n_players, const int32_t* shape /* [P] */, int64_t n_problems,
                   const double* tensors /* [n_problems, P, K_0 .. K_{P-1}] */, const osg_meta_cfg* cfgs, int64_t n_cfgs,
                   const double* initial, double* average, double* last, int on_host);

/* ---- alpha-rank on a batch of normal-form meta-games ------------------------------------------------
 * open_spiel/python/egt/alpharank.py: compute() at a finite alpha (use_fast_compute) or at infinite alpha with one noise
 * level eps, and sweep_pi_vs_epsilon(); psro_v2's default meta-solver.  A problem is P payoff tensors [K_0 .. K_{P-1}], one
 * per player, row-major; the chain's states are the n = K_0 * .. * K_{P-1} pure profiles, a profile's id its row-major
 * index.  n_players = 1 is the single-population chain with the local selection model: `shape` is then the [K, K] of one
 * square table and n = K.  The stationary distribution comes from a Grassmann-Taksar-Heyman elimination, which never
 * subtracts: no negative mass, small masses keep their relative accuracy, and nothing fails where the reference's
 * eigen-solve does.  csrc/osg_alpharank.h has every formula and the one order of every sum (the multiply-add is not
 * fused); a workgroup solves one (problem, eps), the matrix in LDS or in the context's scratch.  The bits of a problem's
 * result depend on its tensors and its cfg, not on its position, on n_problems, on the other problems, on `form`, on
 * `chunk` or on on_host.
 *   cfgs      n_cfgs = 1: one cfg for every problem; n_cfgs = n_problems: problem b runs cfgs[b] (a sweep of alpha or m
 *             over copies of one meta-game, or problems of different modes, is one call).  ALWAYS host memory.
 *   mode      0: finite alpha with population size m; 1: infinite alpha at eps; 2: eps_0 = eps (0: 0.5), eps_{t+1} = 0.5
 *             eps_t, solved until the first t > min_iters with |pi_t - pi_{t-1}| <= 1e-8 + 1e-5 |pi_{t-1}| everywhere.
 *   form      0: the matrix stays in LDS where n * n doubles fit the workgroup's LDS limit (from the device's properties)
 *             beside a vector, and in scratch memory otherwise; 1 / 2 name one (1 where it does not fit:
 *             OSG_ERR_UNSUPPORTED).  Every cfg of a call names the same form and the same chunk.
 *   chunk     mode 2: consecutive epsilons solved per launch, speculatively (0: 8, fewer where the scratch for them would
 *             pass 2^30 bytes); the host waits once per chunk for the count of finished problems, also with on_host = 0.
 *   pi        [n_problems, n]
 *   marginals [n_problems, sum K_p] (n_players = 1: [n_problems, K], pi itself), or NULL: per player and strategy the sum
 *             of pi over the profiles that play it (psro_v2/utils.py get_alpharank_marginals)
 *   eps_used, iterations   [n_problems] or NULL: mode 2: the epsilon of the returned pi and its step t; mode 1: eps, 0;
 *             mode 0: 0, 0
 *   status    [n_problems]: 0; 1: the chain is not irreducible in floating point (a pivot row's sum is 0 or not finite: a
 *             finite-alpha fixation probability underflowed, or a payoff is not finite), which also ends a sweep; 2: the
 *             sweep did not stop before max_iters.  With 1 or 2 the problem's pi and marginals are NaN; the other
 *             problems of the call are unaffected.
 * on_host = 1: tensors and every output are host memory and the call returns when the outputs have arrived; on_host = 0:
 * they are device memory and the launches are enqueued on the context's stream.
 * A refused call writes nothing.  OSG_ERR_INVALID: a null ctx, shape, cfgs, tensors, pi or status, n_problems < 0, n_cfgs
 * neither 1 nor n_problems, a mode outside 0..2, mode 0 with m < 1 or an alpha that is not finite, an eps that is negative
 * or not finite (mode 1: or 0), min_iters < 0 or max_iters < 1, a form outside 0..2 or a negative chunk, or either not the
 * same in every cfg, a size below 1, a table that is not square with n_players = 1.  OSG_ERR_UNSUPPORTED: fewer than 1 or
 * more than 5 players, more than 4096 profiles, more than 2^16 problems, a chunk above 64, max_iters above 4096, form 1 where the matrix does
 * not fit, or problems whose scratch for ONE epsilon each would pass 2^30 bytes (global form: n_problems * n * n * 8). */
typedef struct osg_alpharank_cfg {
  int32_t mode;        /* 0 finite alpha (compute), 1 infinite alpha at one eps, 2 sweep over eps */
  int32_t m;           /* mode 0 */
  double alpha;        /* mode 0 */
  double eps;          /* mode 1: inf_alpha_eps; mode 2: the warm start, 0 = 0.5 */
  int32_t min_iters, max_iters;   /* mode 2; the reference's 10 and 100 */
  int32_t form;        /* 0 by size, 1 LDS, 2 global */
  int32_t chunk;       /* mode 2: epsilons per launch, 0 = the implementation's choice */
} osg_alpharank_cfg;
int osg_alpharank(osg_ctx* ctx, int n_players, const int32_t* shape, int64_t n_problems,
                  const double* tensors /* [n_problems, P, K_0 .. K_{P-1}] */, const osg_alpharank_cfg* cfgs, int64_t n_cfgs,
                  double* pi, double* marginals, double* eps_used, int32_t* iterations, int32_t* status, int on_host);

/* ---- Deep CFR (open_spiel/python/pytorch/deep_cfr.py) --------------------------------------------
 * The networks are the caller's (torch); the device does what the reference does one tree node per interpreter step:
 * the traversals, the sampled advantages and the reservoir appends.  The arithmetic is
 * open_spiel_amd/csrc/osg_deep_cfr.h.
 *
 * osg_cfr_infostate_tensors: State::InformationStateTensor(player of the infostate) of every infostate, in the
 *   solver's infostate order, out [I, info_size] f32 (deep_cfr.py:453,472,495), from one member history each.
 *
 * osg_reservoir: ReservoirBuffer (deep_cfr.py:121-213) on the device.  A row is (infostate index i32, iteration i32,
 *   values f32 [num_actions]): osg_cfr_infostate_tensors rebuilds the tensor the reference stores with each row.
 *   The row with add index n (0-based over the buffer's life, osg_reservoir_clear restarts it) goes to slot n while
 *   n < capacity, else to idx = mulhi64(Rng(seed, n, stream).next(), n + 1) if idx < capacity, else nowhere
 *   (append, :150-182; the reference draws idx with np.random.randint(0, n + 1)).
 * osg_reservoir_append: m rows (device arrays d_info [m], d_values [m, num_actions]; one iteration for all) as m
 *   sequential append calls in row order, bit for bit: of the rows of a call that meet in a slot the last one stays.
 *   Two launches, an integer atomicMax per slot and a copy by the winners; no floating-point atomics.
 * osg_reservoir_sizes: rows held, add calls, capacity.
 * osg_reservoir_sample: d_slots [m] i64 = m distinct filled slots (sample, :184-203, choice(replace=False)): the m
 *   smallest keys Rng(seed, slot, stream).next() over the filled slots, ascending by (key, slot).  m above the rows
 *   held is OSG_ERR_INVALID.
 * osg_reservoir_rows: the rows d_slots [m] i64 names (device), any output may be NULL. */
typedef struct osg_reservoir osg_reservoir;
int osg_cfr_infostate_tensors(osg_cfr* s, float* out /* [I, info_size] */, int on_host);
int osg_reservoir_create(osg_ctx* ctx, int num_actions, int64_t capacity, uint64_t seed, uint64_t stream, osg_reservoir** out);
int osg_reservoir_destroy(osg_reservoir* buf);
int osg_reservoir_sizes(osg_reservoir* buf, int64_t* size, int64_t* add_calls, int64_t* capacity);
int osg_reservoir_clear(osg_reservoir* buf);
int osg_reservoir_append(osg_reservoir* buf, int64_t m, const int32_t* d_info, int32_t iteration, const float* d_values);
int osg_reservoir_sample(osg_reservoir* buf, uint64_t seed, uint64_t stream, int64_t m, int64_t* d_slots);
int osg_reservoir_rows(osg_reservoir* buf, const int64_t* d_slots, int64_t m, int32_t* d_info, int32_t* d_iteration,
                       float* d_values);
/* osg_deep_cfr_traverse: _traverse_game_tree(root, player) (deep_cfr.py:413-481) x trajectories on any osg_cfr object
 *   (its tables are not touched).  d_advantages [I, Amax] f32 (device) holds every infostate's advantage-network
 *   output by action id; the strategy of an infostate (_sample_action_from_advantage, :484-512) is formed once per call.
 *   Trajectory g = first_trajectory + j draws Rng(seed, g, 0).unit() in visiting order, one per chance node and one per
 *   opponent node, by NumPy's choice(p=) rule (:432-433, :466-468).  Advantage rows (:445-460) are appended to adv_buf
 *   and strategy rows (:470-479) to strat_buf (either may be NULL) in the reference's order: trajectories in index
 *   order, a trajectory's advantage rows after the node's children returned, its strategy rows at the visit.
 *   h_counts (may be NULL) [2]: advantage rows, strategy rows of the call.  Synchronises once (the row totals).
 *   Decision nodes wider than 4 actions, action ids beyond Amax and more than 24 traverser nodes on a path are
 *   OSG_ERR_UNSUPPORTED.
 * osg_deep_cfr_staged: the rows of the last osg_deep_cfr_traverse in append order, with the per-trajectory offsets
 *   [trajectories + 1] i64 into them and the draws each trajectory consumed [trajectories] i32 (device outputs, any
 *   may be NULL); sizes (host, may be NULL) [5]: trajectories, advantage rows, strategy rows, and the exact upper
 *   bounds of advantage / strategy rows per trajectory that sized the staging. */
int osg_deep_cfr_traverse(osg_cfr* s, const float* d_advantages, int player, int iteration, uint64_t seed,
                          int64_t first_trajectory, int64_t trajectories, osg_reservoir* adv_buf, osg_reservoir* strat_buf,
                          int64_t* h_counts);
int osg_deep_cfr_staged(osg_cfr* s, int64_t* sizes, int64_t* d_adv_offsets, int32_t* d_adv_info, float* d_adv_values,
                        int64_t* d_strat_offsets, int32_t* d_strat_info, float* d_strat_values, int32_t* d_draws);

/* ---- NFSP (open_spiel/python/pytorch/nfsp.py, dqn.py) ---------------------------------------------
 * The part of Neural Fictitious Self-Play (and, with anticipatory 1, of DQN self-play) that the reference runs at one
 * decision per interpreter step: playing episodes, choosing actions from the two networks, forming DQN transitions and
 * supervised rows and appending them to a ring and a reservoir.  The arithmetic is open_spiel_amd/csrc/osg_nfsp.h.
 *
 * osg_transition_ring: dqn.ReplayBuffer on the device.  A row is (infostate index i32, action id i32, reward f32, next
 *   infostate index i32 — -1 at the end of an episode —, final u8); the reference also stores the next state's tensor
 *   and legal mask, which reach its loss only multiplied by `not final`: whoever forms a batch supplies zeros there.
 *   The row with entry index n (0-based over the ring's life, osg_transition_ring_clear restarts it) goes to slot
 *   n % capacity.
 * osg_transition_ring_append: m rows (device arrays [m]) as m sequential appends in row order; of the rows that meet
 *   in a slot the last stays.  No atomics: row r stays iff r + capacity >= m.
 * osg_transition_ring_sizes: rows held, entry index, capacity.
 * osg_transition_ring_sample: d_slots [m] i64 = m distinct filled slots: the m smallest of the keys
 *   Rng(seed, slot, stream).next(), ascending by (key, slot), as osg_reservoir_sample.
 * osg_transition_ring_rows: the rows d_slots [m] i64 names (device), any output may be NULL. */
typedef struct osg_transition_ring osg_transition_ring;
int osg_transition_ring_create(osg_ctx* ctx, int64_t capacity, osg_transition_ring** out);
int osg_transition_ring_destroy(osg_transition_ring* ring);
int osg_transition_ring_sizes(osg_transition_ring* ring, int64_t* size, int64_t* entry_index, int64_t* capacity);
int osg_transition_ring_clear(osg_transition_ring* ring);
int osg_transition_ring_append(osg_transition_ring* ring, int64_t m, const int32_t* d_info, const int32_t* d_action,
                               const float* d_reward, const int32_t* d_next_info, const uint8_t* d_final);
int osg_transition_ring_sample(osg_transition_ring* ring, uint64_t seed, uint64_t stream, int64_t m, int64_t* d_slots);
int osg_transition_ring_rows(osg_transition_ring* ring, const int64_t* d_slots, int64_t m, int32_t* d_info, int32_t* d_action,
                             float* d_reward, int32_t* d_next_info, uint8_t* d_final);
/* osg_nfsp_collect: `episodes` self-play episodes on any osg_cfr object (its tables are not touched), one launch and
 *   one host wait.  d_q [I, Amax] f32 (device) holds the Q-network output of every infostate (row i from the network
 *   of infostate i's player) and d_avg_probs [I, Amax] f32 its average-policy probabilities by action id (the softmax
 *   over the legal logits: zero at illegal ids); both are frozen for the call.  eps, anticipatory [P] (host) are every
 *   player's exploration rate and anticipatory parameter.  Episode g = first_episode + j draws from Rng(seed, g, 0):
 *   P uniforms for the players' modes (BEST_RESPONSE iff u < anticipatory[p]), then one per chance node (NumPy's
 *   choice(p=)), at a BEST_RESPONSE decision one for the explore test and, if it explores, below(n) for the action, at
 *   an AVERAGE_POLICY decision one for choice(p=) over all Amax ids.  Player p's transitions go to rings[p] and the
 *   supervised rows (infostate, probs f32 [Amax]) of its BEST_RESPONSE decisions to reservoirs[p] (iteration field 0),
 *   in the order of the reference's one-episode-after-another loop; rings, reservoirs or any entry may be NULL: nothing
 *   is committed there.  totals (host, may be NULL) [P, 4]: transitions, supervised rows, steps of the DQN agent (its
 *   decisions + 1 in every BEST_RESPONSE episode) and steps of the NFSP agent (decisions + 1 in every episode).
 *   Served: what osg_deep_cfr_traverse serves, with at most 8 players and 15 decisions of one player on a path; the
 *   rest is OSG_ERR_UNSUPPORTED.
 * osg_nfsp_staged: the rows of the last osg_nfsp_collect in sequence order — player by player, a player's rows by
 *   episode, then by time — with offsets [P * episodes + 1] i64 (entry p * episodes + j: the first row of player p in
 *   episode j), the draws each episode consumed and its modes (bit p: BEST_RESPONSE) [episodes] i32 (device outputs,
 *   any may be NULL); sizes (host, may be NULL) [4 + P]: episodes, transitions, supervised rows, rows staged per
 *   (player, episode), and every player's exact bound. */
int osg_nfsp_collect(osg_cfr* s, const float* d_q, const float* d_avg_probs, const double* eps, const double* anticipatory,
                     uint64_t seed, int64_t first_episode, int64_t episodes, osg_transition_ring* const* rings,
                     osg_reservoir* const* reservoirs, int64_t* totals);
int osg_nfsp_staged(osg_cfr* s, int64_t* sizes, int64_t* d_ring_offsets, int32_t* d_ring_info, int32_t* d_ring_action,
                    float* d_ring_reward, int32_t* d_ring_next_info, uint8_t* d_ring_final, int64_t* d_sl_offsets,
                    int32_t* d_sl_info, float* d_sl_probs, int32_t* d_draws, int32_t* d_modes);

/* ---- multi-GPU exchange step ---------------------------------------------------
 * One process per GPU.  Units shard by global index with no data-path collective; the ONE exchange
 * on the path is external-sampling MCCFR's all-reduce(sum) of the regret / average-policy delta
 * tables per mini-batch (osg_mccfr_sample -> all-reduce of the 2 * I * Amax doubles starting at
 * osg_mccfr_delta_ptrs' regret pointer, the two tables being one allocation -> osg_mccfr_apply_deltas),
 * plus, for root-parallel search on a shared root, the children's visit / reward vectors.  The
 * reference has no distributed runtime (single-threaded C++); these entry points are what a C++
 * host of its shape binds instead of torch.distributed.  RCCL is loaded on first use (dlopen), so
 * single-GPU callers never need it.  The 128-byte id comes from rank 0 (osg_comm_unique_id) and
 * reaches the other ranks out of band (file, socket, MPI, launcher environment), as with
 * ncclGetUniqueId / ncclCommInitRank.  Collectives run in place on the context's stream. */
#define OSG_COMM_ID_BYTES 128
typedef struct osg_comm osg_comm;
int osg_comm_unique_id(void* id_out /* OSG_COMM_ID_BYTES */);
int osg_comm_create(osg_ctx* ctx, int rank, int world, const void* id /* OSG_COMM_ID_BYTES */, osg_comm** out);
int osg_comm_destroy(osg_comm* c);
/* The one-shot all-reduce for the path's latency-bound messages ("prefer a one-shot direct
 * all-reduce (each rank writes its buffer to all 7 peers, reduces locally)" for <= 45 KB): every rank owns a window
 * in its HBM that all peers map through hipIpc; one launch per call pushes the local buffer into every window over
 * xGMI, waits for the peers' pushes and sums the world's slots IN RANK ORDER — all ranks end with bit-identical
 * sums (a ring associates differently per rank).  No RCCL involved.
 *   1. every rank: osg_comm_oneshot_create(ctx, rank, world, max_doubles, &c)   max_doubles <= 32768, world <= 16
 *   2. every rank: osg_comm_oneshot_handle(c, h)  -> OSG_ONESHOT_HANDLE_BYTES bytes; all-gather them out of band
 *      (the channel the ncclUniqueId would travel on), rank order
 *   3. every rank: osg_comm_oneshot_connect(c, all_handles)
 *   4. osg_allreduce_sum_f64 / _i32 / _f64_begin + osg_allreduce_end as with the RCCL kind; osg_comm_destroy.
 * Ranks may share a device (two processes on one GPU map each other's windows just the same), which is how the
 * 1-GPU test box exercises it.  Failure is all-or-nothing per chunk and never silent: a peer that stays SILENT for
 * OSG_ONESHOT_TIMEOUT_MS (default 120 000; the clock restarts with every chunk that arrives, so a late rank is waited
 * for; 0 = no bound) makes the waiting workgroup POISON its chunk of the caller's buffer (NaN / INT32_MIN) instead of
 * leaving local values beside reduced ones, and raises a sticky error that osg_comm_check and every later call on
 * the communicator report.  What the bound is and is not: it bounds the SILENCE of a peer (the clock restarts with
 * every chunk that arrives), so a call can take up to world x OSG_ONESHOT_TIMEOUT_MS before it gives up; the poison and
 * the sticky error are LOCAL to the rank whose wait ran out — peers that received every chunk reduce normally and do
 * not learn of it from the collective — and the int32 poison INT32_MIN is a value, it does not propagate like a NaN.
 * Hence the caller's rule: every rank calls osg_comm_check after the last collective and the ranks AGREE on the result
 * (one more exchange on the channel the handles travelled on) before any of them folds / publishes what the
 * collective produced; open_spiel_amd/distributed.py ShardedMccfr.finish() does that over torch.distributed (a C++ host
 * calls Communicator::CheckHealth() and exchanges the verdict on the channel its handles travelled on).  The reference
 * has no counterpart (no distributed runtime). */
#define OSG_ONESHOT_HANDLE_BYTES 128
int osg_comm_oneshot_create(osg_ctx* ctx, int rank, int world, int64_t max_doubles, osg_comm** out);
int osg_comm_oneshot_handle(const osg_comm* c, void* handle_out /* OSG_ONESHOT_HANDLE_BYTES */);
int osg_comm_oneshot_connect(osg_comm* c, const void* handles /* world x OSG_ONESHOT_HANDLE_BYTES, rank order */);

/* Waits for the collectives issued so far (both streams) and reports a one-shot timeout, if any: call it before
 * trusting a buffer that went through the LAST collective of a job (a timeout is otherwise reported by the next call). */
int osg_comm_check(osg_comm* c);
int osg_comm_rank(const osg_comm* c);
int osg_comm_world(const osg_comm* c);
int osg_allreduce_sum_f64(osg_comm* c, double* d_buf, int64_t n);
int osg_allreduce_sum_i32(osg_comm* c, int32_t* d_buf, int64_t n);
/* The asynchronous form: _begin orders the collective after everything issued on the context's stream so far
 * and runs it on the communicator's own stream; kernels issued on the context's stream between _begin and
 * _end overlap it (they must not touch d_buf); _end makes the context's stream wait for the collective (no
 * host wait).  One collective in flight per communicator. */
int osg_allreduce_sum_f64_begin(osg_comm* c, double* d_buf, int64_t n);
int osg_allreduce_end(osg_comm* c);

#ifdef __cplusplus
}
#endif
#endif /* OSG_ABI_H_ */
