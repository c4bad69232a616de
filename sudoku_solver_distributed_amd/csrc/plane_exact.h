// plane_exact.h -- exact, uncapped completion count of a board whose search
// is cut into tasks and shared over every lane of the grid.
//
// The search is plane_count.h's, none of it changed: pass_ahead, pick_mrv,
// count_step and the 128-byte stack line.  Its leaves are distinct completions
// and every completion is met in exactly one branch (plane_count.h), so the
// sum of the leaves over ANY partition of the tree's open branches is the
// count.  The partition used here is the stack itself: count_step keeps the
// invariant that every level in use still has an untried digit, and a level's
// line holds the planes before its branch, und[] and the digits not yet
// tried.  A line is therefore a self-contained task -- "the subtrees of this
// cell's remaining digits on these planes" -- and at a DEAD verdict (the
// in-flight state is spent) a lane's remaining work is exactly its levels,
// each independent of the others.  Word 31 of a line, unused by the stack,
// carries the board's index when the line travels as a task.
//
// A call is a sequence of rounds, each one launch.  In a round a lane
//   - resumes the stack it parked in the round before, or takes a task: a
//     line of the task ring (it becomes level 0 of the lane's own stack and
//     the search goes on as from a DEAD verdict), or, the ring's readable part
//     handed out, a board not yet started (load_words);
//   - counts its passes; once it has run `slice` of them it takes no new task
//     and stops at its next DEAD verdict (a counted completion is one), before
//     the pop;
//   - then DONATES its levels to the ring when the part written this round is
//     below the fill target and the reservation succeeds (its task ends; the
//     board has depth - 1 more open tasks), or PARKS: its lines stay where
//     they are, depth and board go into its park word;
//   - flushes its `found` into the board's 64-bit count whenever its task
//     ends, is donated or is parked.
// Nothing waits: a reservation is a bounded number of compare-and-swap
// attempts, a failed one changes nothing, and a lane that cannot donate parks.
//
// The bound of a round.  Every pass whose verdict is OPEN or STUCK leaves at
// least one more cell determined (OPEN: a cell became single; STUCK: the step
// fixes the branch cell), a DEAD step restores a level's und[] of at most 81
// cells, and with no cell undetermined the pass answers SOLVED or DEAD.  So a
// run of passes without a DEAD-or-SOLVED verdict is at most 81 long, the
// verdict that closes it is pass 82 at the latest, and a lane runs fewer than
// slice + EXACT_RUN_MAX passes in a round.
//
// The ring.  One ring of `cap` lines, indexed by 64-bit positions that only
// grow: [head0, limit) is this round's queue, read-only, fixed at the launch;
// [limit, tail) is what this round appends, never read before the next
// launch; an append of k lines needs tail + k - head0 <= cap, so no slot that
// may still be read is written.  Tasks a round leaves unclaimed stay queued.
// exact_slot maps a position to its line, exact_advance moves head0 and limit
// on between rounds.
//
// Plain C++ for host and device: the kernel (exact_kernels.hip) and the host
// model (tests/native/exact_host.cpp) run the same functions over their own
// Stack (push / pop / put_entry) and Shared (the ring, the counters) types.
#ifndef SDK_PLANE_EXACT_H
#define SDK_PLANE_EXACT_H

#include "plane_count.h"

namespace plane {

enum { X_CONT = 0, X_DONE = 1, X_STOP = 2, X_FAULT = 3 };
// the longest run of passes up to and including its DEAD-or-SOLVED verdict
enum { EXACT_RUN_MAX = 82 };
enum { EXACT_RESERVE_TRIES = 4 };  // compare-and-swap attempts of one reservation
enum { STACK_BOARD = 31 };         // a task line's board index
// the head block's 64-bit words
enum {
    XH_CLAIM = 0,    // lines of [head0, limit) handed out this round (may overshoot)
    XH_BOARDS = 1,   // boards handed out (may overshoot n)
    XH_TAIL = 2,     // the ring's write position
    XH_OPEN = 3,     // open tasks of the call (boards not yet started included)
    XH_DONATED = 4,  // lines donated
    XH_PARKS = 5,    // lane parks
    XH_MAXPASS = 6,  // the most passes a lane ran in one round
    XH_WORDS = 32
};
enum : uint64_t { X_NO_ROOM = ~(uint64_t)0 };

// One iteration of a lane with a task.  resume: the lane's next step is the
// DEAD step of the deepest level (a task line just taken, or a parked stack);
// no pass is run and no stop is taken, so every task a lane holds advances by
// at least one digit per round.  Otherwise one pass, the completion counted,
// and at a DEAD verdict the task's end (X_DONE: no level left), the round's
// stop (X_STOP: `slice` passes run and levels left; nothing is popped), or the
// step.  X_FAULT: a push past max_depth or a line that breaks the invariant.
template <class Stack>
PS_FN int exact_iter(Board &B, uint32_t (&und)[3], uint32_t (&nd)[3], uint32_t &depth, uint32_t &found,
                     uint32_t &passes, bool &resume, uint32_t slice, const Stack &stk, uint32_t max_depth)
{
    int r = DEAD;
    if (!resume) {
        r = pass_ahead(B, und, nd);
        passes++;
        if (r == OPEN) return X_CONT;
        if (r == SOLVED) {
            found++;
            r = DEAD;  // and look for another
        }
        if (r == DEAD) {
            if (depth == 0) return X_DONE;
            if (passes >= slice) return X_STOP;
        }
    }
    resume = false;
    const int s = count_step(B, und, nd, r, depth, stk, max_depth);
    return s == C_CONT ? X_CONT : s == C_DONE ? X_DONE : X_FAULT;
}

// A stopped lane's levels to the ring, if the round still wants tasks and the
// slots can be reserved (reserved first, written after: a failed reservation
// leaves the ring as it was).  B and und[] are spent and serve as the copy's
// registers.  Shared: wants() -- the part written this round is below the
// fill target; reserve(k) -> first position or X_NO_ROOM; put(position, B,
// und, entry, board).  Returns whether the levels went.
template <class Stack, class Shared>
PS_FN bool exact_donate(Board &B, uint32_t (&und)[3], uint32_t depth, uint32_t board, const Stack &stk,
                        const Shared &sh)
{
    if (!sh.wants()) return false;
    const uint64_t base = sh.reserve(depth);
    if (base == X_NO_ROOM) return false;
    for (uint32_t level = 0; level < depth; ++level) {
        const uint32_t e = stk.pop(level, B, und);
        sh.put(base + level, B, und, e, board);
    }
    return true;
}

// The reservation on the ring's write position `tail` (a: load(p), cas(p,
// expected&, desired)): k lines at the position returned, or X_NO_ROOM with
// nothing changed.
template <class Atomics>
PS_FN uint64_t exact_reserve(const Atomics &a, uint64_t *tail, uint64_t head0, uint64_t cap, uint32_t k)
{
    uint64_t t = a.load(tail);
    for (int i = 0; i < EXACT_RESERVE_TRIES; ++i) {
        if (t + k - head0 > cap) return X_NO_ROOM;
        if (a.cas(tail, t, t + k)) return t;
    }
    return X_NO_ROOM;
}

// The fill target of a grid: the part of the ring a round writes is kept
// below about two lines per lane, so that the next round has a task for every
// lane without every busy lane spilling its stack every round.  A tuning
// constant: results never depend on it.
PS_FN uint64_t exact_fill_target(uint64_t lanes, uint64_t cap)
{
    const uint64_t want = 2 * lanes;
    return want < cap ? want : cap;
}

// Lines of the ring: the two lists of max_tasks lines each (the one a round
// reads, the one it writes) laid end to end; max_tasks 0: four lines a lane.
PS_FN uint64_t exact_ring_lines(uint64_t lanes, uint64_t max_tasks)
{
    return 2 * (max_tasks ? max_tasks : 4 * lanes);
}

// The ring's slot of a position in [head0, head0 + cap), slot0 being head0's
// slot (head0 % cap, kept by exact_advance so that no lane divides): one
// subtraction of cap at the most.
PS_FN uint64_t exact_slot(uint64_t pos, uint64_t head0, uint32_t slot0, uint64_t cap)
{
    uint64_t s = (uint64_t)slot0 + (pos - head0);
    if (s >= cap) s -= cap;
    return s;
}

// Between two rounds, on the host: the lines claimed leave the queue (`claim`
// is the round's XH_CLAIM, which may overshoot the queue's length), what the
// round appended joins it (`tail` is its XH_TAIL).  Keeps head0 <= limit <=
// tail <= head0 + cap and slot0 == head0 % cap.
PS_FN void exact_advance(uint64_t claim, uint64_t tail, uint64_t cap, uint64_t &head0, uint32_t &slot0, uint64_t &limit)
{
    const uint64_t len = limit - head0;
    const uint64_t took = claim < len ? claim : len;
    head0 += took;
    slot0 = (uint32_t)((slot0 + took) % cap);
    limit = tail;
}

// idle lanes before a wave claims tasks (results never depend on it): the
// count's measured choice (count_kernels.hip)
enum { EXACT_REFILL = 16 };

}  // namespace plane

#endif  // SDK_PLANE_EXACT_H
