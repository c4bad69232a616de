// plane_enum.h -- every completion of a board, listed: plane_exact.h's shared
// search with the completion handed out at the SOLVED verdict.
//
// Nothing of the search or of its scheduling is new: pass_ahead, pick_mrv,
// count_step and the stack line (plane_count.h), the tasks, the ring, donate,
// park and the round's bound (plane_exact.h).  The leaves of that search are
// the board's completions, each met in exactly one branch, so over ANY
// partition of the open branches into tasks every completion is met exactly
// once by exactly one lane; at that verdict the lane's planes ARE the grid
// (plane::store_values).  A list that receives every leaf once is therefore
// the completion set, whatever the slice, the ring, the grid or the batch: only
// the order of its rows depends on them.
//
// The list.  One 64-bit cursor (XH_TOTAL, in the head block) hands out rows:
// a completion that is allowed to be listed takes the next value with one
// fetch-add, and writes row `slot` and its owner when slot < capacity.  Slots
// are dense from 0, every slot below min(cursor, capacity) has exactly one
// writer, and a call ends only when every lane has left: rows [0, listed) are
// all written, nothing at or beyond `listed` is, and the cursor's final value is
// `total`, the completions that asked for a slot.
//
// The per-board limit (limit > 0).  The board's 64-bit count becomes a ticket:
// a lane adds one per completion and lists it only when the ticket is below
// `limit`, so never more than `limit` rows of a board ask for a slot; the lane
// that draws the last ticket, or one past it, ends its task, and a lane that
// takes a ring line or resumes a parked stack of a board whose count has
// reached the limit ends that task at once (enum_dropped).  The board's count
// may overshoot by the lanes in flight; the final kernel clamps it
// (enum_final).  Nobody waits for anybody.  With limit 0 a lane keeps its
// completions in `found` and flushes them as plane_exact.h says.
//
// Plain C++ for host and device: the kernel (enum_kernels.hip) and the host
// model (tests/native/enum_host.cpp) run the same functions over their own
// Stack and Out types.
#ifndef SDK_PLANE_ENUM_H
#define SDK_PLANE_ENUM_H

#include "plane_exact.h"

namespace plane {

enum { XH_TOTAL = 7 };  // the head block's list cursor: completions that asked for a slot
enum { ENUM_DONE = 1, ENUM_PARTIAL = 2, ENUM_LIMITED = 3 };

// Has a board with `count` tickets drawn reached its limit?  (limit 0: none)
PS_FN bool enum_reached(uint64_t count, uint64_t limit) { return limit != 0 && count >= limit; }

// A task line just taken or a parked stack resumed (resume) of a board whose
// count has reached the limit: the task is dropped.
PS_FN bool enum_dropped(bool resume, uint64_t count, uint64_t limit) { return resume && enum_reached(count, limit); }

// rows written: the slots below the capacity
PS_FN uint64_t enum_listed(uint64_t total, uint64_t capacity) { return total < capacity ? total : capacity; }

// A completion, the lane's planes still holding it.  Out: ticket(board) ->
// the board's count before this completion (fetch-add of one; limit > 0
// only); slot() -> the cursor before this completion (fetch-add of one);
// write(slot, B, board) -> row and owner.  Returns whether the lane's task
// goes on: false once the board's limit is reached.
template <class Out>
PS_FN bool enum_emit(const Board &B, uint32_t board, uint32_t &found, uint64_t limit, uint64_t capacity, const Out &out)
{
    bool more = true;
    if (limit) {
        const uint64_t t = out.ticket(board);
        if (!(t < limit)) return false;  // past the limit: not listed, not counted (the clamp)
        more = t + 1 < limit;
    } else {
        found++;
    }
    const uint64_t slot = out.slot();
    if (slot < capacity) out.write(slot, B, board);
    return more;
}

// exact_iter with the completion handed to emit(B) -> go on? while the planes
// still hold it.  emit counts it (found or the board's ticket: enum_emit); a
// false answer ends the task with X_DONE, its levels dropped.
template <class Stack, class Emit>
PS_FN int enum_iter(Board &B, uint32_t (&und)[3], uint32_t (&nd)[3], uint32_t &depth, uint32_t &passes, bool &resume,
                    uint32_t slice, const Stack &stk, uint32_t max_depth, Emit emit)
{
    int r = DEAD;
    if (!resume) {
        r = pass_ahead(B, und, nd);
        passes++;
        if (r == OPEN) return X_CONT;
        if (r == SOLVED) {
            if (!emit(B)) return X_DONE;
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

// A board's final answer from its count, its open tasks and its status so far
// (0, SDK_INVALID or SDK_FAULT): the count clamped to the limit.
PS_FN void enum_final(uint64_t &count, int32_t &status, int32_t open, uint64_t limit)
{
    if (status != 0) {
        count = 0;
        return;
    }
    if (enum_reached(count, limit)) {
        count = limit;
        status = ENUM_LIMITED;
    } else {
        status = open == 0 ? ENUM_DONE : ENUM_PARTIAL;
    }
}

}  // namespace plane

#endif  // SDK_PLANE_ENUM_H
