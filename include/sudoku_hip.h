/*
 * sudoku_hip.h -- C ABI of the MI355X (gfx950) Sudoku solver library
 * (libsudoku_hip.so, built from sudoku_solver_distributed_amd/csrc/).
 *
 * Plain pointers and sizes only.  Every `d_*` pointer is DEVICE memory on the
 * calling thread's current HIP device; `stream` is a hipStream_t (NULL = the
 * default stream).  Calls are asynchronous on `stream` unless noted.
 *
 * Grid format: 81 bytes per board, row-major, 0 = empty, 1..9 = digit; a batch
 * of n boards is n*81 contiguous bytes.
 *
 * Caller memory: a uint8_t array may start at any address (no alignment is
 * asked of it); int32_t / int64_t arrays need their natural alignment (4 / 8
 * bytes), a workspace, a scratch and a node state record 16 bytes.  No byte
 * outside the documented extent of an output, scratch or workspace argument
 * is ever written, and an input array is never modified, unless the caller
 * passes it as an output too where that is allowed.  Aliasing an input with
 * an output is allowed only where an entry says so (sdk_solve_batch,
 * sdk_solve_batch_grid, sdk_solve_batches); every other entry needs its
 * arguments disjoint.  (sdk_count_solutions_batch and sdk_count_exact_batch
 * read the aligned dwords that hold a board, so up to 3 bytes on either side
 * of the boards are read; they never change an answer.)
 *
 * Sizes: n is a count of rows, and every offset into an array is formed in 64
 * bits.  Byte extents past 4 GiB are supported and tested (tests/
 * test_gpu_large.py: boards, solutions and lists of 4.0 GiB at 53 025 065 rows,
 * marks of 4.0 GiB at 26 512 921 rows); row indices up to 2^31 - 1.  Row
 * indices beyond that, and int32 / int64 arrays of 2^31 bytes or more (2^29
 * rows), are outside what the tests reach.
 *
 * Return codes: 0 = launched / ok, <0 = error (text in sdk_last_error()).
 *
 * Each entry point replaces one reference interface
 * (cristiano-nicolau/sudoku_solver_distributed):
 */
#ifndef SUDOKU_HIP_H
#define SUDOKU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-board status written by the solvers */
#define SDK_UNSOLVABLE 0  /* gen.py:28 `return False`; output = input board   */
#define SDK_SOLVED 1      /* gen.py:18/25 `return True`; output = filled board */
#define SDK_INVALID -1    /* a byte > 9 in the input (rejected, output = input) */
#define SDK_CANCELLED -2  /* ordered mode: a lower-indexed board already solved */
#define SDK_FAULT -3      /* internal consistency check failed (never expected) */
#define SDK_NO_RETURN -4  /* sdk_peer_solve_batch: node.py's /solve loop never returns */

/* the reference's two walks (cell choice; digits are always tried 1..9) */
#define SDK_ORDER_GEN 0   /* gen.py:6-28: first empty cell of the LAST row that
                             has one (its scan breaks only the inner loop) */
#define SDK_ORDER_NODE 1  /* node.py:62-74: first empty cell, row-major      */

/* Bytes of device workspace sdk_solve_batch needs on the current device:
 * queue heads, cancel word, statistics, and the plane kernel's per-lane DFS
 * stacks and the deferred-board list (about 1.08 GB on an MI355X).  Allocate
 * once per device, zero once;
 * the library re-arms the per-call words itself on `stream`.
 * A workspace is SINGLE-STREAM: every call that passes the same workspace
 * must be issued on the same stream (or ordered by the caller), because each
 * sdk_solve_batch re-arms the workspace's queue head before its kernels when
 * they use it (not for a small unordered batch the static hand-out covers).
 * Enqueueing is thread-safe (the library serialises its launch sequences). */
size_t sdk_workspace_bytes(void);

/* Solve n boards.  For every board the output is the FIRST solution of the
 * reference walk selected by `order`, bit-identical:
 *   SDK_ORDER_GEN  gen.py:6-28          solve_sudoku(board)
 *   SDK_ORDER_NODE node.py:31-40,62-74  SudokuSolver.solve_sudoku, including
 *                  is_valid_move's short-circuit (node.py:44-45: every unit
 *                  sums to 45 -> any digit is accepted; only boards with
 *                  clashing givens can reach it).
 * d_puzzles and d_solutions may alias (the same pointer: an in-place solve;
 * partly overlapping arrays are not allowed).
 * `ordered` != 0 selects frontier mode: once board i is solved, boards j > i
 * are abandoned (status SDK_CANCELLED) and the lowest solved index is kept in
 * the workspace (sdk_read_stats out[4]).
 * sdk_solve_batch, sdk_solve_batch_grid and sdk_solve_batches: byte extents
 * past 4 GiB are supported and tested, out of place and in place, with either
 * kernel; row indices up to 2^31 - 1. */
int sdk_solve_batch(const uint8_t *d_puzzles, uint8_t *d_solutions, int32_t *d_status,
                    int64_t n, void *d_workspace, int order, int ordered, void *stream);

/* sdk_solve_batch with the lane-per-board kernel's grid capped at
 * `grid_waves` waves per SIMD (0: as many as fit, sdk_solve_batch's choice).
 * For launches kept in flight on several streams, each with its own
 * workspace (BatchSolver.solve_inflight): with a grid of 2 waves per SIMD two
 * launches are resident together, so one launch's drain (its last boards,
 * most lanes idle) runs beside the next one's start.  Results never depend on
 * it; a negative value is a bad argument (-2).  Replaces the same reference
 * walks as sdk_solve_batch (gen.py:6-28, node.py:62-74).
 * grid_waves | SDK_GRID_PIPELINED: another launch is queued behind this one
 * on the device.  Its drained waves then finish only their own last boards
 * and exit, so the next launch's waves take their slots; without the flag
 * (the launch's end is the caller's wait) they share their last boards
 * across the XCD through the tail pool (tail mode 2). */
#define SDK_GRID_PIPELINED 0x10000
int sdk_solve_batch_grid(const uint8_t *d_puzzles, uint8_t *d_solutions, int32_t *d_status,
                         int64_t n, void *d_workspace, int order, int ordered, void *stream,
                         int grid_waves);

/* Several independent batches solved by ONE launch sequence on one
 * workspace (unordered): batch i is d_puzzles[i] -> d_solutions[i],
 * d_status[i], n[i] boards, exactly as sdk_solve_batch_grid would solve it
 * alone (same bytes, same statuses).  The lane-per-board kernel's queue runs
 * over the batches laid end to end, so the lanes that finish one batch's
 * boards take the next batch's and the grid drains once per call instead of
 * once per batch: a multi-step persistent launch (bench.py's strong-scaling
 * steps, where one GPU's share of a step is too small to fill the chip).
 * 1 <= count <= SDK_MAX_BATCHES; a batch may be empty; batches must not
 * overlap each other's outputs.  A batch may be solved in place
 * (d_solutions[i] == d_puzzles[i]), as with sdk_solve_batch.  Returns 0 / -1 (HIP error) / -2 (bad
 * arguments).  Replaces the same reference walks as sdk_solve_batch
 * (gen.py:6-28, node.py:62-74), once per board. */
#define SDK_MAX_BATCHES 32
int sdk_solve_batches(const uint8_t *const *d_puzzles, uint8_t *const *d_solutions, int32_t *const *d_status,
                      const int64_t *n, int count, void *d_workspace, int order, void *stream, int grid_waves);

/* Batch Sudoku.check (mode 0, sudoku.py:119-140: every row, column and box
 * sums to 45 and holds 9 distinct values) or node.py's SudokuSolver.check
 * (mode 1, node.py:82-116: sums only).  d_ok[i] = 1/0.  d_ok must not alias
 * d_grids.  sdk_check_batch and sdk_first_candidate_batch: byte extents past
 * 4 GiB are supported and tested; row indices up to 2^31 - 1. */
int sdk_check_batch(const uint8_t *d_grids, int32_t *d_ok, int64_t n, int mode, void *stream);

/* Batch of node.py "solve" tasks (node.py:384-406 -> 76-80,
 * SudokuSolver.solve_sudoku_destributed): d_num[i] = first digit 1..9 that
 * is_valid_move (node.py:42-60) accepts at cell d_cells[i] (= row*9+col) of
 * board i, or 0 for None.  A cell index outside 0..80 gives d_num[i] = -1. */
int sdk_first_candidate_batch(const uint8_t *d_grids, const int32_t *d_cells,
                              int32_t *d_num, int64_t n, void *stream);

/* The reference's HTTP /solve algorithm, node.py:534-557
 * P2PNode.peer_sudoku_solve, one FRESH single node per board (handicap 0, no
 * peers; sdk_peer_solve_seq below carries one node's state across requests):
 * a greedy row-major cell loop with node.py's repair step (node.py:419-532),
 * not a search.  d_out[i] = the board it leaves (valid or not), d_status[i] =
 * SDK_SOLVED (its final check passed), SDK_UNSOLVABLE (returned, check
 * failed), SDK_NO_RETURN (node.py loops forever on this board; d_out = the
 * board at that point) or SDK_INVALID (a byte > 9); d_validations[i] =
 * node.py's `validations` counter after the call (one per
 * SudokuSolver.check: every is_valid_move plus the final check).
 * No two of the arrays may alias (d_out != d_boards), here and in
 * sdk_peer_solve_seq.  sdk_peer_solve_batch: byte extents past 2 GiB are
 * supported and tested; row indices up to 2^31 - 1 (sdk_peer_solve_seq, one
 * lane walking its requests in order, is not tested at such sizes). */
int sdk_peer_solve_batch(const uint8_t *d_boards, uint8_t *d_out, int32_t *d_status, int32_t *d_validations,
                         int64_t n, void *stream);

/* The same /solve loop on ONE P2PNode serving n requests in order
 * (node.py:534-557, requests 0..n-1 as the reference's single-threaded
 * HTTPServer would take them).  The node keeps partial_solution and
 * tried_numbers_by_position (node.py:149, 167) across requests, and a later
 * request's repair step (node.py:501-506) reads what earlier ones left, so
 * request i starts from the state request i-1 left.  d_node_state: one
 * SDK_PEER_STATE_BYTES record in device memory, in/out (all zero = a new
 * node).  Outputs per request as sdk_peer_solve_batch; d_validations[i] is
 * the counter's increase during request i.  A request with a byte > 9 gets
 * SDK_INVALID and leaves the node as it was.  After SDK_NO_RETURN the
 * reference node spins forever and serves nothing more; this call goes on
 * from the state the loop spun in. */
#define SDK_PEER_STATE_BYTES 1600
int sdk_peer_solve_seq(const uint8_t *d_boards, uint8_t *d_out, int32_t *d_status, int32_t *d_validations,
                       int64_t n, void *d_node_state, void *stream);

/* One level of the reference walk's search tree, for splitting a single hard
 * board over waves / GPUs (node.py's per-cell peer task split, node.py:419-449,
 * re-designed as a frontier split).  Every input node is propagated; then
 *   dead   -> no child,
 *   solved -> one child: the solved grid,
 *   open   -> one child per candidate of the walk's next cell (`order`),
 *             digits ascending.
 * A node with a byte > 9 gets no child either (it is not propagated).
 * Children of all nodes, concatenated in input order, are therefore in the
 * walk's (lexicographic) order, and the first SOLVED child of the frontier
 * carries the walk's first solution.
 *   d_tmp:      scratch, n*81 bytes
 *   d_offsets:  n+1 int64; d_offsets[n] = total children (read it back)
 *   d_children: capacity cap*81 bytes; children past cap are not written.
 * Caller checks d_offsets[n] <= cap.
 * Byte extents past 4 GiB (nodes, children) are supported and tested, and so
 * is a level of more than 2^26 nodes, which the library cuts into several
 * launches; row indices up to 2^31 - 1. */
int sdk_expand_frontier(const uint8_t *d_nodes, int64_t n, uint8_t *d_tmp, int64_t *d_offsets,
                        uint8_t *d_children, int64_t cap, int order, void *stream);

/* Copy statistics to host (synchronous on `stream`):
 * out[0] boards finished, out[1] boards solved, out[2] guesses (branch
 * nodes of the searches that gave each board its answer), out[3]
 * propagation passes / sweeps executed (all work, including searches the
 * plane kernel abandoned when it handed a board over), out[4] lowest solved
 * index in ordered mode (INT64_MAX if none), out[5] boards the plane kernel
 * handed to the wave-per-board pass (clashing givens, searches deeper than
 * its stack, the last few boards of a wave once the queue is empty).
 * reset != 0 zeroes them afterwards (and the boards-assigned count of
 * sdk_verify_workspace; never its error word). */
int sdk_read_stats(void *d_workspace, int64_t out[6], int reset, void *stream);

/* Every board answered?  (Synchronous on `stream`; library extension, the
 * reference's walk answers every board it is given, gen.py:6-28.)  Each
 * solve launch adds its board count to the workspace, each board's answer
 * (any status) counts once as finished, and a kernel that could not finish a
 * board it had taken sets an error word (SDK_ERR_* bits: 1 = a tail-pool
 * record it had claimed was never published).  out (may be
 * NULL): out[0] boards assigned, out[1] boards finished, out[2] error bits,
 * all since the last sdk_read_stats(reset) / report; out[3] reserved (0).
 * Returns 0 when
 * assigned == finished and no error bit is set; -3 otherwise (text in
 * sdk_last_error(); the error word is then cleared and the counts re-synced,
 * so each fault is reported once); -1 HIP error; -2 bad arguments. */
int sdk_verify_workspace(void *d_workspace, int64_t out[4], void *stream);

/* The same six counters as sdk_read_stats, copied to DEVICE memory d_out[6]
 * asynchronously on `stream` (stream-ordered with the solves on that
 * workspace: two snapshots around a solve give that solve's own counts
 * without a host synchronisation). */
int sdk_snapshot_stats(const void *d_workspace, int64_t *d_out, void *stream);

/* Solve-kernel selection (library extension, no reference counterpart):
 * SDK_KERNEL_AUTO (default) SDK_KERNEL_PLANE for batches of 8192 boards or
 * more, SDK_KERNEL_PACKED below; SDK_KERNEL_PLANE one lane per board on
 * digit-plane bitboards (boards with clashing givens or very deep searches
 * go to a wave-per-board pass); SDK_KERNEL_PACKED one wavefront per board,
 * both cells of a lane packed in one word.  Both give the same results.
 * 0 restores the default (or $SDK_SOLVE_KERNEL = auto|plane|packed).
 * Returns the previous selection, -1 for an unknown value. */
#define SDK_KERNEL_AUTO 1
#define SDK_KERNEL_PACKED 5
#define SDK_KERNEL_PLANE 6
int sdk_set_solve_kernel(int kernel);

/* Plane-kernel tuning (library extension, no reference counterpart; the
 * defaults are the measured optimum).  refill: idle lanes
 * before a wave refills; tail: active lanes at or below which a drained wave
 * hands its last boards to the tail solver (0 off, at most 40); tail_mode: 1
 * the wave-wide solver continues each search on the wave itself, 2 the same
 * through a per-XCD pool that every exiting wave of the XCD drains; chunk:
 * most boards a wave claims from the queue at once (at
 * most 64: a claim is staged and converted in one go; 0 one claim per refill).  A
 * negative value keeps that knob; all four negative restore the defaults
 * ($SDK_PLANE_REFILL / _TAIL / _TAIL_MODE / _CHUNK).  Results never depend on
 * them.  Returns 0, or -1 for an out-of-range value (nothing changed). */
int sdk_set_plane_tuning(int refill, int tail, int tail_mode, int chunk);

/* Plane-kernel search (library extension, no reference counterpart): a
 * board still searching after `mrv_after` propagation passes goes back to
 * its propagated root and counts its completions (to two) branching on
 * fewest-candidates cells: exactly one completion is the walk's answer, none
 * means none for the walk too, two send the board back to the walk's own
 * branch order.  With the switch on, a board whose
 * propagated root keeps >= 58 open cells counts from the root at once.  0
 * keeps every board on the walk's order; -1
 * restores the default ($SDK_PLANE_MRV, built-in 128).  Results never
 * depend on it.  Returns the setting in effect before the call (the
 * default's value when no override was set), -2 for an out-of-range value
 * (nothing changed). */
int sdk_set_plane_search(int mrv_after);

/* Count the completions of n boards, capped (library extension, no reference
 * counterpart: the reference only ever asks for one completion):
 *   d_count[i] = min(limit, number of completions of board i that are valid
 *                Sudoku grids -- every row, column and box holds 1..9 once,
 *                the givens kept),   1 <= limit <= SDK_COUNT_MAX_LIMIT.
 * A board whose givens repeat a digit in a row, column or box has count 0.
 * This deliberately DIFFERS from sdk_solve_batch: the reference walk never
 * tests the givens and may "solve" such a board; the count is about valid
 * grids only.  A byte > 9 gives SDK_INVALID in d_count[i]; SDK_FAULT would
 * mean the search outgrew its stack, which 81 levels make impossible.
 * d_first (may be NULL, must not alias d_puzzles): per board 81 bytes -- for
 * count >= 1 a completion, the first one the count's search met (for
 * count == 1 necessarily the walk's answer); for count <= 0 the input board.
 * d_scratch: at least sdk_count_scratch_bytes(n, max_waves) bytes of device
 * memory, contents irrelevant: the call re-arms its queue head itself on
 * `stream`.  A scratch is SINGLE-STREAM like a workspace; the solve
 * workspace, its counters and sdk_verify_workspace are not involved.
 * max_waves caps the kernel's grid (0: as many waves as fit on the device at
 * the kernel's occupancy); results never depend on it.  The scratch holds the
 * per-lane search stacks of min(ceil(n / 64), waves) waves, about 660 KB per
 * wave: little for a small call, about 2.7 GB for a full grid on an MI355X.
 * The limit bounds the work per completion found, not the work to prove
 * that a sparse board has none.
 * Asynchronous on `stream`.  Returns 0 / -1 (HIP error) / -2 (bad arguments:
 * limit out of range, negative n or max_waves, a NULL pointer that is
 * required, scratch too small), by return code only (sdk_last_error() is not
 * set); arguments are checked before any launch and n == 0 returns 0.
 * sdk_count_scratch_bytes returns 0 for negative arguments; for every other n
 * up to INT64_MAX it is exactly 256 + min(ceil(n / 64), waves) * 64 * 81 * 128.
 * Byte extents past 4 GiB (puzzles, d_first) are supported and tested; row
 * indices up to 2^31 - 1. */
#define SDK_COUNT_MAX_LIMIT 1024
size_t sdk_count_scratch_bytes(int64_t n, int max_waves);
int sdk_count_solutions_batch(const uint8_t *d_puzzles, int32_t *d_count, uint8_t *d_first /* NULL ok */,
                              int64_t n, int limit, void *d_scratch, size_t scratch_bytes,
                              int max_waves, void *stream);

/* Canonical form of n boards under Sudoku's symmetries (library extension, no
 * reference counterpart).  A board is 81 bytes 0..9; whether it obeys the
 * rules plays no part.  A line permutation p in [0, 1296) is
 * p = ((bp*6 + a)*6 + b)*6 + d with PERM3 = {012, 021, 102, 120, 201, 210}:
 *   perm_p[k] = 3*PERM3[bp][k/3] + PERM3[(a, b, d)[k/3]][k%3].
 * Symmetry sym = (t*1296 + ri)*1296 + ci, t in {0, 1}, R = perm_ri,
 * C = perm_ci: image cell (i, j) = g[R[i]][C[j]] for t == 0, g[C[j]][R[i]]
 * for t == 1; the image's non-zero digits are then relabelled 1, 2, ... in
 * order of first appearance in row-major order, zeros stay zero.
 *   d_canon[i] = the lexicographically smallest image of board i over all
 *                SDK_CANON_SYMMETRIES sym (bytes compared 0 < 1 < ... < 9),
 *   d_sym[i]   = the smallest sym whose image it is,
 *   d_autos[i] = the number of sym whose image it is (for a valid grid the
 *                order of its automorphism group within this group).
 * Two boards are the same puzzle under these symmetries exactly when their
 * canonical forms are equal.  A board with a byte > 9 comes back as it is,
 * with SDK_INVALID in d_sym[i] and d_autos[i].  d_autos may be NULL; d_canon
 * must not alias d_boards.
 * slices: every board's search is cut into that many parts, one workgroup
 * each (1..SDK_CANON_MAX_SLICES); 0 picks enough of them for a small batch
 * to fill the device (1 for a large batch).  Results never depend on it.
 * d_scratch: at least sdk_canonical_scratch_bytes(n, slices) bytes of device
 * memory (64 bytes per board and slice), contents irrelevant; SINGLE-STREAM
 * like a workspace.  The solve workspace is not involved.
 * Asynchronous on `stream`.  Returns 0 / -1 (HIP error) / -2 (bad arguments:
 * slices out of range, negative n, a NULL pointer that is required, d_canon
 * == d_boards, scratch too small), by return code only; arguments are
 * checked before any launch and n == 0 returns 0.
 * sdk_canonical_scratch_bytes returns 0 for negative or out-of-range
 * arguments, and for an n whose 64 * n * slices bytes do not fit size_t (the
 * batch entry refuses such an n).
 * A scratch past 4 GiB (25 891 boards and more at 2592 slices) is supported and
 * tested: the library cuts a batch into launches of fewer than 2^32 threads. */
#define SDK_CANON_SYMMETRIES 3359232
#define SDK_CANON_MAX_SLICES 2592
size_t sdk_canonical_scratch_bytes(int64_t n, int slices);
int sdk_canonical_batch(const uint8_t *d_boards, uint8_t *d_canon, int32_t *d_sym, int32_t *d_autos /* NULL ok */,
                        int64_t n, int slices /* 0 = auto */, void *d_scratch, size_t scratch_bytes,
                        void *stream);

/* Rate n puzzles: how much logic each one needs (library extension, no
 * reference counterpart).  A board is 81 bytes 0..9.  Its state is a set of
 * candidates per cell -- a given v starts as {v}, an empty cell as {1..9} --
 * and the rules only remove candidates:
 *   N  a cell with the one candidate d removes d from its 20 peers;
 *   H  a digit with exactly one place in a row, column or box becomes that
 *      cell's only candidate;
 *   L  locked candidates: where a box and a row or column meet in three
 *      cells that hold a place of d, and d has no other place in the box
 *      (the line), d leaves the rest of the line (the box);
 *   T  for a cell with two or more candidates and one of them, d: if the
 *      {N, H, L} closure of the state with that cell fixed to d is dead, d
 *      leaves the cell (one level of trial, never nested).
 * A state is dead when a cell has no candidate or a unit has no place for a
 * digit; solved when every cell has one candidate and it is not dead.  Level
 * 1 is {N}, 2 {N, H}, 3 {N, H, L}, 4 {N, H, L, T}; closure_L is the level's
 * rules applied until nothing changes.  The rules are monotone, so closure_L
 * does not depend on the order they fire in.  For
 * 1 <= max_level <= SDK_RATE_MAX_LEVEL:
 *   d_rating[i]       = the lowest L <= max_level with closure_L solved; else
 *                       0 when closure_max_level is dead (no completion
 *                       exists: the rules are sound); else max_level + 1;
 *   d_open[4 i + L-1] = the cells of closure_L without exactly one candidate;
 *                       0 from the solving level on, -1 where closure_L is
 *                       dead, SDK_RATE_NOT_RUN for L > max_level;
 *   d_marks[81 i + c] = the candidates of cell c, bit d-1 for digit d, in the
 *                       deepest closure computed (closure_rating when solved:
 *                       the completion; else closure_max_level); all zero
 *                       when that closure is dead.
 * Givens that repeat a digit in a unit have rating 0 (N empties both cells).
 * A byte > 9 gives SDK_INVALID in d_rating[i] and all four d_open entries,
 * and zero marks.  d_open and d_marks may be NULL; d_marks needs 2-byte
 * alignment, d_boards none.  Inputs are never modified and no byte outside
 * these extents is written.
 * d_scratch: at least sdk_rate_scratch_bytes(n, max_level) bytes of device
 * memory, 8-byte aligned, contents irrelevant: the call re-arms its counters
 * itself on `stream` (256 bytes, and at max_level 4 eight bytes per board:
 * the list of the boards level 3 leaves open).  SINGLE-STREAM like a
 * workspace; the solve workspace is not involved.
 * Asynchronous on `stream`.  Returns 0 / -1 (HIP error) / -2 (bad arguments:
 * max_level out of range, n negative or above 2^31 - 1, a NULL pointer that
 * is required, a misaligned pointer, scratch too small), by return code only;
 * arguments are checked before any launch and n == 0 returns 0.
 * sdk_rate_scratch_bytes returns 0 for bad arguments (n above 2^31 - 1 among
 * them).  Byte extents past 4 GiB (d_marks) are supported and tested; row
 * indices up to 2^31 - 1. */
#define SDK_RATE_MAX_LEVEL 4
#define SDK_RATE_NOT_RUN -2
size_t sdk_rate_scratch_bytes(int64_t n, int max_level);
int sdk_rate_batch(const uint8_t *d_boards, int32_t *d_rating, int32_t *d_open /* n*4, NULL ok */,
                   uint16_t *d_marks /* n*81, NULL ok */, int64_t n, int max_level, void *d_scratch,
                   size_t scratch_bytes, void *stream);

/* Named techniques: which of the human rules -- singles, locked candidates,
 * subsets, fish -- n states fall to (library extension, no reference
 * counterpart).  The state, dead and solved, and the rules N,
 * H and L are sdk_rate_batch's.  The Hall step of size k on a 9x9 0/1 matrix
 * with row sets M[0..8]: for every k-subset I of rows, with u the union of
 * its rows, |u| < k makes the state dead (pigeonhole) and |u| == k takes u
 * out of every row outside I; rows of any size take part.
 *   S_k  subsets, k = 2, 3, 4: in each of the 27 units the step on cells x
 *        candidate digits (naked pairs, triples, quads) and on digits x the
 *        cells where the digit has a place (hidden ones);
 *   F_k  fish, k = 2, 3, 4: for each digit the step on rows x the columns
 *        where it has a place and on columns x rows (X-wing, swordfish,
 *        jellyfish, both orientations).
 * Every rule only removes candidates and is monotone with dead as the bottom
 * state, so the fixpoint of a rule set depends on no order.
 * A rule set is a bit mask of SDK_LOGIC_N .. SDK_LOGIC_F4; `ladder` (HOST
 * memory, read before the call returns) holds `steps` of them, 1 <= steps <=
 * SDK_LOGIC_MAX_STEPS, each with SDK_LOGIC_N and a proper superset of the one
 * before; closure_j is the fixpoint of step j's rules, or dead.  The default
 * ladder is {N, N|H, N|H|L, +S2, +S3|S4, +F2, +F3|F4}: singles, hidden
 * singles, locked candidates, pairs, triples / quads, X-wing, swordfish /
 * jellyfish, and step 8: beyond.
 * State i starts as board i's start state (d_boards NULL: every board empty)
 * ANDed with the pencil marks d_start[81 i + c] (bit d-1 for digit d;
 * d_start NULL: every mask 0x1FF).  Both NULL is a bad argument.
 *   d_step[i]         = the lowest j (1-based) with closure_j solved; 0 when
 *                       some computed closure is dead; steps + 1 otherwise;
 *   d_open[8 i + j-1] = the cells of closure_j without exactly one candidate;
 *                       0 from the solving step on, -1 from the dead step
 *                       on, SDK_LOGIC_NOT_RUN past `steps`;
 *   d_left[8 i + j-1] = the candidates closure_j leaves over all 81 cells; 81
 *                       from the solving step on, -1 from the dead step on,
 *                       SDK_LOGIC_NOT_RUN past `steps` (d_open does not see
 *                       a removal that empties no cell);
 *   d_marks[81 i + c] = the candidates of cell c in the deepest closure
 *                       computed; all zero when that closure is dead.
 * A byte > 9 or a mark with a bit above 0x1FF gives SDK_INVALID in d_step[i]
 * and all eight d_open and d_left entries, and zero marks.  d_open, d_left
 * and d_marks may be NULL; d_start and d_marks need 2-byte alignment,
 * d_boards none.  Inputs are never modified and no byte outside these
 * extents is written.
 * d_scratch: at least sdk_logic_scratch_bytes(n, steps) bytes of device
 * memory, 8-byte aligned, contents irrelevant: the call re-arms its counters
 * itself on `stream` (256 bytes, and eight bytes per board: the list of the
 * boards the leading N / N|H / N|H|L steps leave open).  SINGLE-STREAM like a
 * workspace; the solve workspace is not involved.
 * Asynchronous on `stream`.  Returns 0 / -1 (HIP error) / -2 (bad arguments:
 * steps out of range, a mask outside 0x1FF or without N, a step that is not a
 * proper superset of the one before, both inputs NULL, n negative or above
 * 2^31 - 1, a NULL pointer that is required, a misaligned pointer, scratch
 * too small), by return code only; arguments are checked before any launch
 * and n == 0 returns 0 once n and the ladder are checked.
 * sdk_logic_scratch_bytes returns 0 for bad arguments (n above 2^31 - 1 among
 * them). */
#define SDK_LOGIC_MAX_STEPS 8
#define SDK_LOGIC_NOT_RUN -2
#define SDK_LOGIC_N 1
#define SDK_LOGIC_H 2
#define SDK_LOGIC_L 4
#define SDK_LOGIC_S2 8
#define SDK_LOGIC_S3 16
#define SDK_LOGIC_S4 32
#define SDK_LOGIC_F2 64
#define SDK_LOGIC_F3 128
#define SDK_LOGIC_F4 256
size_t sdk_logic_scratch_bytes(int64_t n, int steps);
int sdk_logic_batch(const uint8_t *d_boards /* NULL ok */, const uint16_t *d_start /* NULL ok */,
                    const uint32_t *ladder /* HOST memory, `steps` words */, int steps,
                    int32_t *d_step, int32_t *d_open /* n*8, NULL ok */, int32_t *d_left /* n*8, NULL ok */,
                    uint16_t *d_marks /* n*81, NULL ok */, int64_t n,
                    void *d_scratch, size_t scratch_bytes, void *stream);

/* The solving path of n states: every deduction, round by round (library
 * extension, no reference counterpart).  State, start state
 * (board ANDed with the pencil marks; d_boards NULL: empty boards, d_start
 * NULL: masks of 0x1FF, both NULL refused), dead and solved are
 * sdk_logic_batch's.  `rules` is one mask of SDK_LOGIC_N .. SDK_LOGIC_F4 that
 * holds N; the nine CLASSES, in order, are its bit indices: 0 N, 1 H, 2 L,
 * 3 S2, 4 S3, 5 S4, 6 F2, 7 F3, 8 F4.
 * A FIRING is one of
 *   a Hall firing (m, I, u): on matrix m (0..71, 9 kind + idx: kind 0 the row
 *     fish of digit idx, rows x columns; 1 the column fish, columns x rows;
 *     2..4 hidden in row / column / box idx, digits x cells; 5..7 naked in row
 *     / column / box idx, cells x digits; the cells of a box row by row) a
 *     k-subset I of rows (a row mask) with union u and |u| == k.  Its action:
 *     u leaves every row outside I.  Class N is size 1 on the naked matrices
 *     45..71 (a cell with one candidate d: d leaves the unit's other cells; a
 *     single fires once per unit it lies in), class H size 1 on the hidden
 *     matrices 18..44 (a digit with one place in a unit: the cell loses its
 *     other digits), class S_k size k on 18..71, class F_k size k on 0..17;
 *   an L firing (dir, d, line, box): line 0..8 a row, 9..17 a column, meeting
 *     the box; digit d has a place in the three shared cells and, dir 0
 *     (pointing), no other place in the box: d leaves the rest of the line;
 *     dir 1 (claiming), no other place in the line: d leaves the rest of the
 *     box.
 * A firing is EFFECTIVE on a state when its action removes at least one
 * candidate there; `removed` is how many.  A VIOLATION is a k-subset with
 * |u| < k; the size-1 violations (an empty row of a matrix 18..71) are the
 * rating's dead and are always checked, whatever `rules` is.
 * The schedule of one board, r = 0 rounds done:
 *   1 the state is dead: stop, SDK_PATH_DEAD, with one contradiction event:
 *     class 0, round r + 1, removed 0, the smallest (m, I) among the matrices
 *     18..71 with an empty row, u = 0;
 *   2 the state is solved: stop, SDK_PATH_SOLVED;
 *   3 max_rounds > 0 and r == max_rounds: stop, SDK_PATH_LIMITED;
 *   4 the classes of `rules` in ascending order: an S_k or F_k with a
 *     violation stops the board, SDK_PATH_DEAD, with a contradiction event of
 *     that class, the smallest (m, I) and its u; the first class with an
 *     effective firing is the round's class; no class fires: SDK_PATH_STUCK;
 *   5 ++r; every effective firing of the round's class is one event of round
 *     r, all evaluated on the round's start state; the new state is the start
 *     state minus the union of their removals.
 * (m, I) compares m first, then I as a number.  Every round removes a
 * candidate: at most 648 rounds.  The end state is the fixpoint of `rules` on
 * the start state, or dead (the rules are monotone), and the
 * path uses no class above the lowest prefix of classes whose closure solves
 * the board.  The events are covariant under every symmetry of the state.
 *   row k of d_rows = four words, one 16-byte store a row:
 *     word 0  the owner (the board's index);
 *     word 1  round (bits 0..15), class (16..19), bit 20 set for a
 *             contradiction event, removed (24..31);
 *     word 2  a Hall event: m | I << 8 | u << 17; an L event: m = 72 + dir,
 *             I = 1 << (d - 1), u = line | box << 5;
 *     word 3  the candidates left over all 81 cells after the event's round;
 *             for a contradiction event the count before the round.
 * Rows [0, listed) are all written, without holes; nothing at or beyond row
 * `listed` is written.  The ORDER of the rows is unspecified; the SET is
 * reproducible.
 *   d_info (DEVICE memory, 2 values) = {total, listed = min(total, capacity)};
 *   rows beyond the capacity are dropped (which ones is unspecified) and the
 *   call still returns 0.  capacity == 0 is a pure count (d_rows may be NULL).
 *   d_count[i]      = board i's events, the contradiction event included,
 *                     whatever the capacity;
 *   d_rounds[i]     = the rounds done;
 *   d_status[i]     = SDK_PATH_DEAD, SDK_PATH_SOLVED, SDK_PATH_STUCK or
 *                     SDK_PATH_LIMITED; SDK_INVALID for a byte above 9 or a
 *                     mark bit above 0x1FF: count 0, no rounds, no row;
 *   d_hist[9 i + c] = the events of class c, contradiction events not counted;
 *   d_marks[81 i+c] = the end state, all zero when DEAD or invalid.
 * d_hist and d_marks may be NULL.  d_rows needs 16-byte alignment, d_info 8,
 * d_count, d_rounds, d_status and d_hist 4, d_start and d_marks 2, d_boards
 * none.  Inputs are never modified and no byte outside these extents is
 * written.
 * d_scratch: at least sdk_path_scratch_bytes(n, max_waves) bytes of device
 * memory (64: the board head and the row cursor), 8-byte aligned, contents
 * irrelevant: the call re-arms its heads itself on `stream`.  SINGLE-STREAM
 * like a workspace; the solve workspace is not involved.  max_waves > 0 caps
 * the kernel's grid (0: the device's waves at the kernel's occupancy); results
 * never depend on it.  Asynchronous on `stream`: two launches ordered by the
 * stream alone.  Returns 0 / -1 (HIP error) / -2 (bad arguments: a mask
 * outside 0x1FF or without N, max_rounds, capacity or max_waves negative, a
 * capacity above INT64_MAX / 16 (its bytes would not fit an int64), n
 * negative or above 2^31 - 1, both inputs NULL, a NULL pointer that is
 * required, a misaligned pointer, scratch too small), by return code only;
 * arguments are checked before any launch and n == 0 returns 0 once the
 * scalars are checked.  sdk_path_scratch_bytes returns 0 for bad arguments.
 * Row arithmetic is 64-bit throughout; a list past 4 GiB is not yet tested. */
#define SDK_PATH_DEAD 0
#define SDK_PATH_SOLVED 1
#define SDK_PATH_STUCK 2
#define SDK_PATH_LIMITED 3
size_t sdk_path_scratch_bytes(int64_t n, int max_waves);
int sdk_path_batch(const uint8_t *d_boards /* NULL ok */, const uint16_t *d_start /* NULL ok */,
                   uint32_t rules, int max_rounds, int64_t n,
                   uint32_t *d_rows /* capacity*4, NULL ok iff capacity == 0 */, int64_t capacity,
                   int32_t *d_count /* n */, int32_t *d_rounds /* n */, int32_t *d_status /* n */,
                   int32_t *d_hist /* n*9, NULL ok */, uint16_t *d_marks /* n*81, NULL ok */,
                   int64_t *d_info /* DEVICE, 2 values */,
                   void *d_scratch, size_t scratch_bytes, int max_waves, void *stream);

/* The exact candidates of n boards (library extension, no reference
 * counterpart).  A completion of a board is a valid Sudoku grid -- every row,
 * column and box holds 1..9 once -- that keeps the givens.
 *   d_marks[81 i + c] = the digits that at least one completion of board i
 *                       puts into cell c, bit d-1 for digit d (the format of
 *                       sdk_rate_batch's marks): a given's own bit when the
 *                       board has a completion, all zero when it has none;
 *   d_count[i]        = min(2, completions): 0 for zero marks, 1 when every
 *                       cell has one bit (the marks are the completion), 2
 *                       otherwise.
 * The answer is exact, with no cap and no truncated case: it does not depend
 * on any search order and the marks of a symmetry image of a board are the
 * image of its marks.  sdk_rate_batch's marks are a superset of these.  The
 * work is one capped count and then at most one first-completion search per
 * candidate still unwitnessed, not an enumeration.
 * A board whose givens repeat a digit in a row, column or box has no
 * completion: zero marks, count 0.  A byte > 9 gives zero marks and
 * SDK_INVALID in d_count[i]; SDK_FAULT (with zero marks) would mean a search
 * outgrew its stack, which 81 levels make impossible.
 * d_count may be NULL.  d_marks needs 2-byte alignment (d_count 4), d_boards
 * none.  Inputs are never modified, no byte outside these extents is written,
 * and the arguments are disjoint.
 * d_scratch: at least sdk_candidates_scratch_bytes(n, max_waves) bytes of
 * device memory, 8-byte aligned, contents irrelevant: the call re-arms its
 * queue head itself on `stream`.  SINGLE-STREAM like a workspace; the solve
 * workspace, its counters and sdk_verify_workspace are not involved.
 * max_waves caps the kernel's grid (0: as many waves as fit on the device at
 * the kernel's occupancy); results never depend on it.  The scratch holds 256
 * bytes and, per wave of min(ceil(n / 64), waves), 64 lanes x 83 lines x 128
 * bytes (about 680 KB: little for a small call, about 2.8 GB for a full grid
 * on an MI355X).
 * Asynchronous on `stream`.  Returns 0 / -1 (HIP error) / -2 (bad arguments:
 * negative n or max_waves, a NULL pointer that is required, a misaligned
 * pointer, scratch too small), by return code only (sdk_last_error() is not
 * set); arguments are checked before any launch and n == 0 returns 0.
 * sdk_candidates_scratch_bytes returns 0 for negative arguments.  Byte
 * extents past 4 GiB (d_marks) are supported and tested; row indices up to
 * 2^31 - 1. */
size_t sdk_candidates_scratch_bytes(int64_t n, int max_waves);
int sdk_candidates_batch(const uint8_t *d_boards, uint16_t *d_marks /* n*81 */, int32_t *d_count /* n, NULL ok */,
                         int64_t n, void *d_scratch, size_t scratch_bytes, int max_waves, void *stream);

/* Redundant givens of n boards: minimise a puzzle, or probe which of its
 * clues it could lose (library extension, no reference counterpart).  A
 * completion is what sdk_count_solutions_batch counts: a valid Sudoku grid
 * that keeps the givens.
 *   d_status[i] = min(2, completions of board i); clashing givens give 0, a
 *                 byte > 9 SDK_INVALID; SDK_FAULT would mean a search outgrew
 *                 its stack, which 81 levels make impossible, and gives
 *                 out = input, never a partial result.
 * For every status but 1, d_out row i is the input row and d_removed[i] = 0.
 * Status 1, SDK_MIN_GREEDY: P starts as the board.  The turns run t = 0..80
 * with c = d_order[81 i + t], or c = t when d_order is NULL.  A turn is
 * skipped when c > 80 or P[c] == 0; the loop ends once P has max_empty or more
 * zero cells (the input's own zeros count); otherwise P[c] is erased if P
 * without it still has exactly one completion.  d_out row i = the final P,
 * d_removed[i] = the givens erased.  With max_empty = 81 and an order that
 * names every given the result is a minimal proper puzzle.  d_order needs no
 * validation: repeats and bytes above 80 are harmless by the skip rule.
 * 0 <= max_empty <= 81.
 * Status 1, SDK_MIN_PROBE: d_order and max_empty are not read.  Every given
 * is tested alone against the INPUT board; d_out row i = the board with every
 * individually redundant given erased (the clues every proper sub-puzzle must
 * keep; in general not a proper puzzle itself), d_removed[i] = how many were
 * erased.  A puzzle is minimal exactly when d_removed[i] == 0.
 * Each test is one first-completion search of the puzzle with the cell opened
 * to every digit but its own, not a count.
 * d_order and d_removed may be NULL.  d_out must not alias d_boards; all
 * arguments are disjoint.  Byte arrays may start at any address, the int32
 * arrays need 4-byte alignment.  Inputs are never modified and no byte outside
 * these extents is written.
 * d_scratch: at least sdk_minimize_scratch_bytes(n, max_waves) bytes of device
 * memory, 8-byte aligned, contents irrelevant: the call re-arms its queue head
 * itself on `stream`.  SINGLE-STREAM like a workspace; the solve workspace,
 * its counters and sdk_verify_workspace are not involved.  max_waves caps the
 * kernel's grid (0: as many waves as fit on the device at the kernel's
 * occupancy); results never depend on it.  The scratch holds 256 bytes and,
 * per wave of min(ceil(n / 64), waves), 64 lanes x 82 lines x 128 bytes.
 * Asynchronous on `stream`.  Returns 0 / -1 (HIP error) / -2 (bad arguments:
 * a mode or max_empty out of range, negative n or max_waves, a NULL pointer
 * that is required, a misaligned pointer, scratch too small, d_out ==
 * d_boards), by return code only (sdk_last_error() is not set); arguments are
 * checked before any launch and n == 0 returns 0 before any other check.
 * sdk_minimize_scratch_bytes returns 0 for negative arguments.  Byte extents
 * past 4 GiB (d_boards, d_order, d_out) are supported and tested; row indices
 * up to 2^31 - 1. */
#define SDK_MIN_GREEDY 0
#define SDK_MIN_PROBE 1
size_t sdk_minimize_scratch_bytes(int64_t n, int max_waves);
int sdk_minimize_batch(const uint8_t *d_boards, const uint8_t *d_order /* n*81, NULL ok */, uint8_t *d_out /* n*81 */,
                       int32_t *d_status /* n */, int32_t *d_removed /* n, NULL ok */, int64_t n, int mode,
                       int max_empty, void *d_scratch, size_t scratch_bytes, int max_waves, void *stream);

/* A random completion of every item: random full grids, random grids that
 * contain a pattern of givens, another solution of an ambiguous board (library
 * extension, no reference counterpart).  A completion is what
 * sdk_count_solutions_batch counts: a valid Sudoku grid that keeps the givens.
 * Items: items = n * per_board, 1 <= per_board, items <= 2^31 - 1.  Item q
 * samples board q / per_board under key = first_key + q (mod 2^64) and writes
 * row q of d_out and d_status[q].  An item's answer is a function of its
 * board's 81 bytes, seed and key alone: not of max_waves, of the batch it came
 * in or of its place in it, so a batch may be cut anywhere and continued with
 * first_key moved on.
 *   d_status[q] = 1  a completion was found: row q is a valid grid that keeps
 *                    the givens
 *                 0  the board has none (givens that repeat a digit in a unit
 *                    included): row q is the input board
 *                 SDK_INVALID  a byte > 9: row q is the input board
 *                 SDK_FAULT    the search outgrew its stack, which 81 levels
 *                    make impossible: row q is the input board, never a
 *                    partial grid
 * d_boards == NULL: every board is empty, no board byte is read, and the
 * status is always 1 (random full grids).
 * The rule, so that a caller can restate it.  The search is the count's: the
 * library's propagation to a fixpoint; there, a branch on a fewest-candidates
 * cell (the cell choice is deterministic); at a contradiction, back to the
 * deepest branch that has a digit left; the first completion met is the
 * answer.  Only the digit of a branch is random -- out of the cell's
 * candidates on a new branch, out of the branch's remaining digits on a
 * return to it.  With all arithmetic mod 2^64 and `mask` the digits to choose
 * from (bit d-1 for digit d):
 *     mix(x):   x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;
 *               x *= 0x94D049BB133111EB;  x ^= x >> 31
 *     h       = mix(mix(seed) + key)
 *     r_t     = mix(h + (t + 1) * 0x9E3779B97F4A7C15)
 *                   t = 0, 1, 2, ... counts this item's choices so far; every
 *                   choice advances t, also when the mask has one bit
 *     index   = ((r_t >> 32) * popcount(mask)) >> 32
 *     digit   = the index-th lowest set bit of mask
 * What this is and what it is not.  Each branch picks uniformly among the
 * digits left in the cell.  Every completion of the board has positive
 * probability: choosing a completion's own digit at every branch never dies,
 * because the rules only remove digits that no completion uses.  The
 * distribution over completions is that of a randomised search; it is NOT
 * uniform.  The search is complete: status 0 is a proof that there is none.
 * d_out must not alias d_boards; all arguments are disjoint.  d_boards and
 * d_out may start at any address, d_status needs 4-byte alignment.  Inputs are
 * never modified and no byte outside these extents is written.
 * d_scratch: at least sdk_sample_scratch_bytes(items, max_waves) bytes of
 * device memory, 8-byte aligned, contents irrelevant: the call re-arms its
 * queue head itself on `stream`.  SINGLE-STREAM like a workspace; the solve
 * workspace, its counters and sdk_verify_workspace are not involved.
 * max_waves caps the kernel's grid (0: as many waves as fit on the device at
 * the kernel's occupancy); results never depend on it.  The scratch holds 256
 * bytes and, per wave of min(ceil(items / 64), waves), 64 lanes x 81 lines x
 * 128 bytes.
 * Asynchronous on `stream`.  Returns 0 / -1 (HIP error) / -2 (bad arguments:
 * negative n or max_waves, per_board < 1, more than 2^31 - 1 items, a NULL
 * d_out, d_status or d_scratch, a misaligned d_status or d_scratch, d_out ==
 * d_boards, scratch too small), by return code only (sdk_last_error() is not
 * set); arguments are checked before any launch and n == 0 returns 0 before
 * any other check.  sdk_sample_scratch_bytes returns 0 for negative
 * arguments.  Byte extents past 4 GiB (d_out) are supported and tested, with
 * per_board > 1 and with keys that wrap past 2^64 inside the batch; item
 * indices up to 2^31 - 1. */
size_t sdk_sample_scratch_bytes(int64_t items, int max_waves);
int sdk_sample_batch(const uint8_t *d_boards /* n*81, NULL = every board empty */, uint8_t *d_out /* items*81 */,
                     int32_t *d_status /* items */, int64_t n, int per_board, uint64_t seed, uint64_t first_key,
                     void *d_scratch, size_t scratch_bytes, int max_waves, void *stream);

/* The unique candidates of n boards: which clue, added to a board, makes it a
 * proper puzzle (library extension, no reference counterpart).  A completion
 * is what sdk_count_solutions_batch counts: a valid Sudoku grid that keeps
 * the givens.  For board i, cell c and digit d:
 *   d_once[81 i + c]  bit d-1 is set when EXACTLY one completion puts d into
 *                     c.  For an empty cell: the board with the clue (c, d)
 *                     added has exactly one completion.  A given's own bit is
 *                     set exactly when the board has exactly one completion.
 *   d_marks[81 i + c] bit d-1 is set when at least one completion puts d into
 *                     c: byte for byte what sdk_candidates_batch writes, so
 *                     once is a subset of marks;
 *   d_count[i]        = min(2, completions), as sdk_candidates_batch.
 * The answer is exact, with no cap and no truncated case: it does not depend
 * on any search order, and the arrays of a symmetry image of a board are the
 * images of its arrays.  Why it is exact: the leaves of one depth-first
 * search are distinct completions.  A first search from the givens records
 * every placement it meets (W) and every placement two of its completions
 * share (V); if it ends before a fixed number of completions, marks = W and
 * once = W & ~V.  Otherwise, for every placement (c, d) of the propagated
 * board R that is not yet in V or settled, one search of R with c fixed to d
 * counts to two: none removes the placement from R; one, then exhaustion,
 * settles it as "exactly one"; two completions T1, T2 put T1 & T2 into V.  V
 * only ever receives placements that two distinct completions share, a
 * placement is settled only by an exhaustive search, and the loop ends only
 * when every placement of R is in V or settled: marks = R, once = R & ~V.  (A
 * completion met in one search is never paired with one met in another: they
 * may be the same grid.)  DESIGN.md §18.
 * A board whose givens repeat a digit in a row, column or box has no
 * completion: zero arrays, count 0.  A byte > 9 gives zero arrays and
 * SDK_INVALID in d_count[i]; SDK_FAULT (with zero arrays, never a partial
 * answer) would mean a search outgrew its stack, which 81 levels make
 * impossible.
 * d_marks and d_count may be NULL.  d_once and d_marks need 2-byte alignment
 * (d_count 4), d_boards none.  Inputs are never modified, no byte outside
 * these extents is written, and the arguments are disjoint.
 * d_scratch: at least sdk_unique_candidates_scratch_bytes(n, max_waves) bytes
 * of device memory, 8-byte aligned, contents irrelevant: the call re-arms its
 * queue head itself on `stream`.  SINGLE-STREAM like a workspace; the solve
 * workspace, its counters and sdk_verify_workspace are not involved.
 * max_waves caps the kernel's grid (0: as many waves as fit on the device at
 * the kernel's occupancy); results never depend on it.  The scratch holds
 * exactly 256 bytes and, per wave of min(ceil(n / 64), waves), 64 lanes x 85
 * lines x 128 bytes (696 320 bytes a wave).
 * Asynchronous on `stream`.  Returns 0 / -1 (HIP error) / -2 (bad arguments:
 * negative n or max_waves, a NULL pointer that is required, a misaligned
 * pointer, scratch too small), by return code only (sdk_last_error() is not
 * set); arguments are checked before any launch and n == 0 returns 0.
 * sdk_unique_candidates_scratch_bytes returns 0 for negative arguments.  Byte
 * extents past 4 GiB (d_once, d_marks) are supported and tested; row indices
 * up to 2^31 - 1. */
size_t sdk_unique_candidates_scratch_bytes(int64_t n, int max_waves);
int sdk_unique_candidates_batch(const uint8_t *d_boards, uint16_t *d_once /* n*81 */,
                                uint16_t *d_marks /* n*81, NULL ok */, int32_t *d_count /* n, NULL ok */,
                                int64_t n, void *d_scratch, size_t scratch_bytes, int max_waves, void *stream);

/* Count the completions of n boards exactly, without a cap (library extension,
 * no reference counterpart).  A completion is what
 * sdk_count_solutions_batch counts: a valid grid that keeps the givens.  The
 * search tree of a board is cut into tasks on the GPU and shared over every
 * lane of the grid, so one heavy board uses the whole device.
 *   d_status[i] == SDK_EXACT_DONE:    d_count[i] is the exact number of
 *       completions of board i.  Givens that repeat a digit in a row, column
 *       or box give 0 with SDK_EXACT_DONE: an exact zero, as in the capped
 *       count.
 *   d_status[i] == SDK_EXACT_PARTIAL: the call ran max_rounds rounds and the
 *       board still had open tasks.  d_count[i] is the number of distinct
 *       completions met so far: a true lower bound, NOT reproducible from run
 *       to run (it depends on which lanes got how far).
 *   d_status[i] == SDK_INVALID:       a byte > 9; d_count[i] = 0.
 *   d_status[i] == SDK_FAULT:         a search outgrew its stack, which 81
 *       levels make impossible; d_count[i] = 0, never a partial number.
 * Boards that finished are unaffected by boards that did not.  For a board
 * with SDK_EXACT_DONE the answer never depends on slice, max_tasks,
 * max_waves, max_rounds, the batch the board came in or its place in it.
 * The call is a sequence of rounds, each one launch of the same grid.  In a
 * round a lane runs about `slice` propagation passes (fewer than slice + 82:
 * it stops at its first dead end past `slice`), then hands the open levels of
 * its search to a task list for the next round, or keeps them when the list
 * is full.  No lane or wave ever waits for another, so every launch is
 * bounded by construction.  max_tasks: the capacity of each of the two task
 * lists (the one a round reads, the one it writes; they share one ring), 0:
 * four tasks per lane of the grid; at most 2^31 - 1.  max_waves: the grid, the
 * same for every n (0: as many waves as fit on the device at the kernel's
 * occupancy).
 * d_count cannot overflow: a completion costs at least one propagation pass
 * of one lane, a call runs fewer than max_rounds * (slice + 82) passes a
 * lane, and a call whose max_rounds * (slice + 82) * 64 * waves reaches 2^63
 * is refused as a bad argument (with a full grid of 2^18 lanes that leaves
 * max_rounds * slice up to about 2^45, years of device time).
 * SYNCHRONOUS on `stream`, like sdk_read_stats: after every round the call
 * reads one 64-byte line of counters back (the number of open tasks decides
 * whether another round runs), and it returns when the results are written.
 * Thread-safe: the library runs one such launch sequence at a time.
 * stats (HOST memory, may be NULL) receives four values: rounds launched,
 * task lines donated, lane parks (a lane kept its levels because the list had
 * no room), and the most passes any lane ran in one round.
 * d_count needs 8-byte alignment, d_status 4, d_boards none.  Inputs are never
 * modified, no byte outside these extents is written, and the arguments are
 * disjoint.  Like the capped count, the call reads the aligned dwords that
 * hold a board, so up to 3 bytes on either side of d_boards are read; they
 * never change an answer.
 * d_scratch: at least sdk_count_exact_scratch_bytes(n, max_waves, max_tasks)
 * bytes of device memory, 16-byte aligned, contents irrelevant: the call arms
 * it itself on `stream`.  SINGLE-STREAM like a workspace; the solve workspace,
 * its counters and sdk_verify_workspace are not involved.  With W waves and
 * T = max_tasks (or 256 W for 0) the scratch holds exactly
 *   256 + W * 64 * 81 * 128 + 2 T * 128 + W * 64 * 8 + 4 n rounded up to 16
 * bytes: the counters, the lanes' stack lines, the task lines, the lanes'
 * park words, the boards' open-task counters.  About 2.9 GB for a full grid
 * of 4096 waves.
 * Returns 0 / -1 (HIP error) / -2 (bad arguments: slice < 1, max_rounds < 1,
 * max_tasks out of range, a pass budget of 2^63, negative n or max_waves, n > 2^31 - 1, a NULL
 * pointer that is required, a misaligned pointer, scratch too small), by
 * return code only (sdk_last_error() is not set); arguments are checked
 * before any launch and n == 0 returns 0 before any other check.
 * sdk_count_exact_scratch_bytes returns 0 for bad arguments (n above 2^31 - 1
 * among them).  The entry has no array that reaches 2^31 bytes below 2^28
 * boards and is not tested at such sizes. */
#define SDK_EXACT_DONE 1    /* d_count[i] is the exact number of completions */
#define SDK_EXACT_PARTIAL 2 /* the round budget ran out: d_count[i] is a lower bound */
size_t sdk_count_exact_scratch_bytes(int64_t n, int max_waves, int64_t max_tasks);
int sdk_count_exact_batch(const uint8_t *d_boards, int64_t *d_count /* n */, int32_t *d_status /* n */,
                          int64_t n, int slice, int max_rounds, int64_t max_tasks, void *d_scratch,
                          size_t scratch_bytes, int max_waves, void *stream,
                          int64_t *stats /* HOST, 4 values, NULL ok */);

/* List every completion of n boards (library extension, no reference
 * counterpart).  A completion is what
 * sdk_count_solutions_batch counts: a valid grid that keeps the givens.  The
 * search is sdk_count_exact_batch's, shared over every lane of the grid in
 * rounds of fewer than slice + 82 passes a lane, with the same task ring and
 * the same meaning of slice, max_rounds, max_tasks and max_waves; its leaves
 * are the completions, each met once, and every one a lane meets and is
 * allowed to list goes to ONE list shared by the whole call:
 *   row k of d_grids = 81 bytes 1..9, d_owner[k] = the board it completes.
 * Rows [0, listed) are all written, without holes; no byte at or beyond row
 * `listed` is written.  The ORDER of the rows is unspecified and differs from
 * run to run; the SET is reproducible: for a board with SDK_ENUM_DONE in a
 * call that did not overflow, the set of its rows never depends on slice,
 * max_tasks, max_waves, max_rounds, capacity, limit, the batch or the board's
 * place in it.
 * info (HOST memory, may be NULL) receives six values: rounds launched, task
 * lines donated, lane parks, the most passes any lane ran in one round,
 * `total` = the completions that asked for a row, `listed` = min(total,
 * capacity).  When total > capacity the rows beyond the capacity are DROPPED
 * (which ones is unspecified); they are still counted in d_count and the call
 * still returns 0: the caller sees listed < total and may call again with
 * capacity = total.  capacity == 0 is a pure count: d_count and d_status are
 * sdk_count_exact_batch's (d_grids and d_owner may then be NULL).
 *   d_status[i] == SDK_ENUM_DONE:    the search of board i ran out; d_count[i]
 *       is its exact number of completions, and without an overflow all of
 *       them are listed.  Givens that repeat a digit in a unit: 0, DONE.
 *   d_status[i] == SDK_ENUM_LIMITED: only with limit > 0: board i has AT LEAST
 *       `limit` completions; d_count[i] == limit, exactly `limit` distinct
 *       completions of it asked for a row and the rest of its search was
 *       dropped.  A board with exactly `limit` completions is LIMITED too
 *       (ask for limit + 1 to tell).  The limit is strict: never more than
 *       `limit` rows of one board ask for a row, so capacity >= n * limit
 *       cannot overflow.  limit == 0: no limit.
 *   d_status[i] == SDK_ENUM_PARTIAL: max_rounds ran out; d_count[i] is the
 *       number of distinct completions met, all of which asked for a row: a
 *       lower bound, not reproducible.
 *   d_status[i] == SDK_INVALID:      a byte > 9; d_count[i] = 0, no row.
 *   d_status[i] == SDK_FAULT:        a search outgrew its stack, which 81
 *       levels make impossible; d_count[i] = 0; rows of that board already
 *       listed may remain, to be discarded by status.
 * SYNCHRONOUS on `stream` and thread-safe like sdk_count_exact_batch: the
 * library runs one such launch sequence at a time.  d_count needs 8-byte
 * alignment, d_status and d_owner 4, d_boards and d_grids none.  Inputs are
 * never modified, no byte outside these extents is written, the arguments are
 * disjoint, and up to 3 bytes on either side of d_boards are read without
 * ever changing an answer.
 * d_scratch: at least sdk_enumerate_scratch_bytes(n, max_waves, max_tasks)
 * bytes of device memory, 16-byte aligned, contents irrelevant, SINGLE-STREAM.
 * With W waves and T = max_tasks (or 256 W for 0) it holds exactly
 *   256 + W * 64 * 81 * 128 + 2 T * 128 + W * 64 * 8 + 4 n rounded up to 16
 * bytes, the exact count's layout.
 * Returns 0 / -1 (HIP error) / -2 (bad arguments: those of
 * sdk_count_exact_batch, and capacity < 0, capacity > 2^31 - 1, limit < 0,
 * capacity > 0 with d_grids or d_owner NULL or d_owner misaligned), by return
 * code only; arguments are checked before any launch and n == 0 returns 0
 * before any other check.  sdk_enumerate_scratch_bytes returns 0 for bad
 * arguments (n above 2^31 - 1 among them).  A list past 4 GiB (d_grids: 54 M
 * rows) is supported and tested; row indices up to 2^31 - 1. */
#define SDK_ENUM_DONE 1    /* the board's search ran out: d_count[i] is exact */
#define SDK_ENUM_PARTIAL 2 /* the round budget ran out: d_count[i] is a lower bound */
#define SDK_ENUM_LIMITED 3 /* the board has at least `limit` completions: d_count[i] == limit */
size_t sdk_enumerate_scratch_bytes(int64_t n, int max_waves, int64_t max_tasks);
int sdk_enumerate_batch(const uint8_t *d_boards, int64_t n,
                        uint8_t *d_grids /* capacity*81, NULL ok iff capacity == 0 */,
                        int32_t *d_owner /* capacity,    NULL ok iff capacity == 0 */,
                        int64_t capacity, int64_t limit /* 0 = none */,
                        int64_t *d_count /* n */, int32_t *d_status /* n */,
                        int slice, int max_rounds, int64_t max_tasks,
                        void *d_scratch, size_t scratch_bytes, int max_waves, void *stream,
                        int64_t *info /* HOST, 6 values, NULL ok */);

/* The smallest backdoors of n puzzles (library extension, no reference
 * counterpart).  Item i is a board b (81 bytes 0..9) and a
 * grid g (81 bytes 1..9) that is a valid Sudoku grid and keeps b's givens;
 * the call has a level L in 1..SDK_BACKDOOR_MAX_LEVEL -- sdk_rate_batch's rule
 * sets {N}, {N, H}, {N, H, L} -- and 1 <= max_size <= SDK_BACKDOOR_MAX_SIZE.
 * For a set S of cells, b + S is b with b[c] = g[c] for c in S; S is a
 * BACKDOOR when closure_L(b + S) is solved (it is then g: the rules are
 * sound).  The rules are monotone, so every superset of a backdoor is one,
 * and a minimum backdoor holds only cells that closure_L(b) leaves with two
 * or more candidates.
 *   d_size[i]           = the smallest |S| of a backdoor, 0..max_size (0
 *                         exactly when sdk_rate_batch rates b 1..L at
 *                         max_level L); max_size + 1 when no set of at most
 *                         max_size cells is one; SDK_INVALID for a byte > 9
 *                         in b or outside 1..9 in g; else
 *                         SDK_BACKDOOR_MISMATCH when g is not a valid grid or
 *                         does not keep b's givens;
 *   d_count[i]          = how many backdoors have exactly that size (at most
 *                         C(81, 4) = 1 663 740): 1 for size 0 (the empty
 *                         set), 0 for max_size + 1 and the negative codes;
 *   d_first[4 i .. + 3] = the lexicographically smallest backdoor of that
 *                         size, cells ascending, 0xFF in the unused places;
 *                         all 0xFF when there is none or the size is 0;
 *   d_cover[81 i + c]   = 1 when cell c lies in at least one backdoor of that
 *                         size, else 0.
 * The answer depends on (b, g, L, max_size) alone: not on the grid size,
 * max_waves, how the subsets are sliced, or the batch.  Size and count are
 * the same for every symmetry image of (b, g) and the cover is the image of
 * the cover; d_first is deterministic but NOT covariant (the smallest set of
 * the image is not the image of the smallest set).  The size does not grow
 * with L.  A board with several completions is legal: its backdoors are those
 * that pin g.  d_count, d_first and d_cover may be NULL; d_size and d_count
 * need 4-byte alignment, the byte arrays none.  Inputs are never modified and
 * no byte outside these extents is written.
 * d_scratch: at least sdk_backdoor_scratch_bytes(n, max_size, max_waves) bytes
 * of device memory (256 + 320 n: a record for every board the level leaves
 * open), 8-byte aligned, contents irrelevant: the call re-arms its counters
 * itself on `stream`.  SINGLE-STREAM like a workspace; the solve workspace is
 * not involved.  max_waves > 0 caps every kernel's grid (0: the device's
 * waves at the kernel's occupancy); results never depend on it.
 * Asynchronous on `stream`: one launch per size 1..max_size between a first
 * and a last one, ordered by the stream alone.  Returns 0 / -1 (HIP error) /
 * -2 (bad arguments: level or max_size out of range, n negative or above
 * 2^31 - 1, max_waves negative, a NULL pointer that is required, a misaligned
 * pointer, scratch too small), by return code only; arguments are checked
 * before any launch and n == 0 returns 0.  sdk_backdoor_scratch_bytes returns
 * 0 for bad arguments.  Row arithmetic is 64-bit throughout; byte extents
 * past 4 GiB (d_boards, d_grids, d_cover: 53 M rows) are not yet tested. */
#define SDK_BACKDOOR_MAX_LEVEL 3
#define SDK_BACKDOOR_MAX_SIZE 4
#define SDK_BACKDOOR_MISMATCH -2
size_t sdk_backdoor_scratch_bytes(int64_t n, int max_size, int max_waves);
int sdk_backdoor_batch(const uint8_t *d_boards, const uint8_t *d_grids, int32_t *d_size,
                       int32_t *d_count /* n, NULL ok */, uint8_t *d_first /* n*4, NULL ok */,
                       uint8_t *d_cover /* n*81, NULL ok */, int64_t n, int level, int max_size,
                       void *d_scratch, size_t scratch_bytes, int max_waves, void *stream);

/* The unavoidable sets of n solution grids (library extension, no reference
 * counterpart).  Input i is a full grid g (81 bytes 1..9); the
 * call has a size m = max_size, 4 <= m <= SDK_UA_MAX_SIZE.
 *   A NEIGHBOUR of g is a valid grid g' != g; D(g') = {c : g'[c] != g[c]}.
 *   Two cells c, c' of D are LINKED when they are peers (they share a row,
 *   column or box) and g'[c] == g[c'] or g[c] == g'[c'].  A neighbour is
 *   CONNECTED when D is connected under links.
 *   A ROW is one connected neighbour with |D| <= m, as the 81-bit set D.  The
 *   rows of g form a MULTISET: two neighbours with the same D give two rows.
 * A neighbour that is not connected is a union of smaller connected ones, and
 * every MINIMAL unavoidable set of at most m cells (a set inside which some
 * neighbour differs from g, no proper subset of which is one) is the D of a
 * row; the rows no other row's D is a proper subset of are exactly the minimal
 * unavoidable sets of at most m cells (sdk_unavoidable_minimal_batch).
 *   row k of d_rows = four words {m0, m1, m2, owner}: cell c is bit c & 31 of
 *   word c >> 5, owner the grid's index.  One 16-byte store a row.
 * Rows [0, listed) are all written, without holes; nothing at or beyond row
 * `listed` is written.  The ORDER of the rows is unspecified and differs from
 * run to run; the MULTISET is reproducible and depends on (g, m) alone.
 *   d_info (DEVICE memory, 2 values) = {total, listed = min(total, capacity)};
 *   when total > capacity the rows beyond the capacity are dropped (which ones
 *   is unspecified) and the call still returns 0.  capacity == 0 is a pure
 *   count (d_rows may then be NULL).
 *   d_count[i]  = the rows of grid i, whatever the capacity;
 *   d_status[i] = SDK_UA_DONE, or SDK_INVALID for a byte outside 1..9, else
 *                 SDK_UA_NOT_A_GRID when a digit repeats in a row, column or
 *                 box; the last two give count 0 and no row.
 * d_rows needs 16-byte alignment, d_info 8, d_count and d_status 4, d_grids
 * none.  Inputs are never modified and no byte outside these extents is
 * written.
 * d_scratch: at least sdk_unavoidable_scratch_bytes(n, max_waves) bytes of
 * device memory (64 + 128 n: nine digit masks a grid), 8-byte aligned,
 * contents irrelevant: the call re-arms its heads itself on `stream`.
 * SINGLE-STREAM like a workspace; the solve workspace is not involved.
 * max_waves > 0 caps every kernel's grid (0: the device's waves at the
 * kernel's occupancy); results never depend on it.  Asynchronous on `stream`:
 * three launches ordered by the stream alone.  Returns 0 / -1 (HIP error) /
 * -2 (bad arguments: max_size out of range, n negative or above 2^31 - 1,
 * capacity negative, max_waves negative, a NULL pointer that is required, a
 * misaligned pointer, scratch too small), by return code only; arguments are
 * checked before any launch and n == 0 returns 0.
 * sdk_unavoidable_scratch_bytes returns 0 for bad arguments.  Row arithmetic
 * is 64-bit throughout; a list past 4 GiB is not yet tested.
 *
 * sdk_unavoidable_minimal_batch: rows (four words each, the fourth ignored)
 * already grouped in CSR form, group j the rows [d_offsets[j], d_offsets[j+1]).
 *   d_keep[k] = 1 exactly when no row of k's group is a proper subset of row
 *   k and no row of lower index in the group equals row k; else 0.
 * No scratch; asynchronous on `stream`; d_rows needs 16-byte alignment,
 * d_offsets 8.  Returns 0 / -1 / -2 (groups negative or above 2^31 - 1,
 * max_waves negative, a NULL or misaligned pointer); groups == 0 returns 0. */
#define SDK_UA_MAX_SIZE 16
#define SDK_UA_DONE 1
#define SDK_UA_NOT_A_GRID -2
size_t sdk_unavoidable_scratch_bytes(int64_t n, int max_waves);
int sdk_unavoidable_batch(const uint8_t *d_grids, int64_t n, int max_size,
                          uint32_t *d_rows /* capacity*4, NULL ok iff capacity == 0 */, int64_t capacity,
                          int32_t *d_count /* n */, int32_t *d_status /* n */,
                          int64_t *d_info /* DEVICE, 2 values */,
                          void *d_scratch, size_t scratch_bytes, int max_waves, void *stream);
int sdk_unavoidable_minimal_batch(const uint32_t *d_rows, const int64_t *d_offsets /* groups+1 */,
                                  int64_t groups, uint8_t *d_keep, int max_waves, void *stream);

/* The k-cell hitting sets of n families of cell sets (library extension, no
 * reference counterpart).  Family i is the cell sets
 * d_sets[d_offsets[i] .. d_offsets[i+1]) -- rows of four words {m0, m1, m2,
 * ignored}, as sdk_unavoidable_batch writes them; only cells 0..80 of a set
 * count -- an ALLOWED mask A = d_allowed[4 i ..] and a REQUIRED mask R =
 * d_required[4 i ..] (three words and an ignored fourth each).  The call has a
 * size k, 0 <= k <= SDK_HIT_MAX_CLUES.
 *   A ROW of family i is a cell set S with R <= S <= A, |S| = k and
 *   S & U != 0 for every set U of the family.
 * The rows of a family form a SET, each S listed once; they depend on (the
 * family's sets as a set of masks, A, R, k) alone, not on the order of the
 * sets, on repeated sets or on max_waves.  So a set with no allowed cell that
 * R does not hit (an all-zero mask among them) gives no row, an empty family
 * gives every C(|A \ R|, k - |R|) filling, and k < |R| or k > |A| gives none.
 *   row j of d_rows = four words {m0, m1, m2, owner}: cell c is bit c & 31 of
 *   word c >> 5, owner the family's index.  One 16-byte store a row.
 * Rows [0, listed) are all written, without holes; nothing at or beyond row
 * `listed` is written.  The ORDER of the rows is unspecified.
 *   d_info (DEVICE memory, 2 values) = {total, listed = min(total, capacity)};
 *   when total > capacity the rows beyond the capacity are dropped (which ones
 *   is unspecified) and the call still returns 0.  capacity == 0 is a count
 *   (d_rows may then be NULL); with limit == 0 as well the search adds a
 *   binomial where the clues left are free instead of walking the fillings.
 *   A count that does not fit an int64 is unspecified.
 *   limit > 0 stops a family after `limit` rows: d_count[i] == limit and the
 *   status is SDK_HIT_LIMITED; which rows are listed is unspecified, each is a
 *   row by the definition.  limit == 0: no limit.
 *   d_count[i]  = the rows of family i, whatever the capacity;
 *   d_status[i] = SDK_HIT_DONE, SDK_HIT_LIMITED, or SDK_INVALID when A or R
 *                 has a bit at or above 81, R is not inside A, or the family's
 *                 offsets descend or span 2^31 sets or more: count 0, no row.
 * d_sets, d_allowed, d_required and d_rows need 16-byte alignment, d_offsets,
 * d_count and d_info 8, d_status 4.  d_sets may be NULL when every family is
 * empty.  Inputs are never modified and no byte outside these extents is
 * written.
 * d_scratch: at least sdk_hitting_sets_scratch_bytes(n, max_waves) bytes of
 * device memory (64: the task head and the row cursor), 8-byte aligned,
 * contents irrelevant: the call re-arms its heads itself on `stream`.
 * SINGLE-STREAM like a workspace; the solve workspace is not involved.
 * max_waves > 0 caps every kernel's grid (0: the device's waves at the
 * kernel's occupancy); results never depend on it.  Asynchronous on `stream`:
 * three launches ordered by the stream alone.  Returns 0 / -1 (HIP error) /
 * -2 (bad arguments: k out of range, n negative or above 2^31 - 1, limit,
 * capacity or max_waves negative, a NULL pointer that is required, a
 * misaligned pointer, scratch too small), by return code only; arguments are
 * checked before any launch and n == 0 returns 0.
 * sdk_hitting_sets_scratch_bytes returns 0 for bad arguments.  Arithmetic is
 * 64-bit throughout. */
#define SDK_HIT_MAX_CLUES 32
#define SDK_HIT_DONE 1
#define SDK_HIT_LIMITED 2
size_t sdk_hitting_sets_scratch_bytes(int64_t n, int max_waves);
int sdk_hitting_sets_batch(const uint32_t *d_sets, const int64_t *d_offsets /* n+1 */,
                           const uint32_t *d_allowed /* n*4 */, const uint32_t *d_required /* n*4 */,
                           int64_t n, int k, int64_t limit,
                           uint32_t *d_rows /* capacity*4, NULL ok iff capacity == 0 */, int64_t capacity,
                           int64_t *d_count /* n */, int32_t *d_status /* n */,
                           int64_t *d_info /* DEVICE, 2 values */,
                           void *d_scratch, size_t scratch_bytes, int max_waves, void *stream);

/* Library / device info. */
const char *sdk_last_error(void);
const char *sdk_version(void);
int sdk_device_cu_count(void);

#ifdef __cplusplus
}
#endif
#endif /* SUDOKU_HIP_H */
