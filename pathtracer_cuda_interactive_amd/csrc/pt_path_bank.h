// pt_path_bank.h — wave-uniform bookkeeping of the register path bank of trace_kernel_v2 (pt_kernels.h).
//
// A wave generates path starts 64 at a time, one per lane at full width, into a few "bank" registers per lane, and its
// scheduler phases hand them out to the lanes whose paths ended.  This header holds only the scalar side of that: which
// work items the bank holds and which slots have been handed out.  It needs no HIP header, so the CPU test
// tests/native/path_bank_check.cpp runs the same code against a simulated work feed.
//
// The bank is filled from the front of the wave's reserved chunk [cur, end) and right-aligned: after a fill of m <= 64 items
// slot s (= lane s) in [64 - m, 64) holds item cur - 64 + s, with cur already moved past the m items.  Nothing moves cur or
// changes the band while the bank holds items (the wave reserves again only with an empty bank), so one scalar, the number
// of slots left, is the whole state: the slots left are [64 - left, 64), and their band is the feed's.
//
// Invariant: every work item a wave has reserved is either in [cur, end) or in a slot [64 - left, 64) of that wave's bank,
// and a banked item leaves only through bank_take of the same wave.  So a wave may stop only when bank_work_left is false,
// and then nothing it reserved is left anywhere.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_BANK_HD __host__ __device__ inline
#else
#define PT_BANK_HD inline
#endif

namespace ptl {

constexpr uint32_t kBankSlots = 64;     // one slot per lane of a wave

struct PathBank {
    uint32_t left;      // slots not yet handed out: [kBankSlots - left, kBankSlots)
};

PT_BANK_HD void bank_init(PathBank& b) { b.left = 0; }

// The bank is empty and the reserved chunk [cur, end) is not: move its first min(64, end - cur) items into the bank.
// Returns the number of slots filled.
PT_BANK_HD uint32_t bank_fill(PathBank& b, uint32_t& cur, uint32_t end) {
    const uint32_t avail = end - cur;
    const uint32_t m = avail < kBankSlots ? avail : kBankSlots;
    b.left = m;
    cur += m;
    return m;
}

// Region-local work item of `slot`, from the feed's cur as bank_fill left it.  Meaningful for the slots of the last fill
// only; for the others the unsigned arithmetic wraps to an item that does not exist.
PT_BANK_HD uint32_t bank_item(uint32_t cur, uint32_t slot) { return cur - kBankSlots + slot; }

// Hands out k = min(n_need, left) slots: the lane of rank r < k takes slot first + r (< kBankSlots).  Returns k.
PT_BANK_HD uint32_t bank_take(PathBank& b, uint32_t n_need, uint32_t& first) {
    const uint32_t k = n_need < b.left ? n_need : b.left;
    first = kBankSlots - b.left;
    b.left -= k;
    return k;
}

// False only when the wave holds no item any more and can reserve none: bank empty, chunk empty, every band exhausted.
PT_BANK_HD bool bank_work_left(const PathBank& b, bool feed_exhausted, uint32_t cur, uint32_t end) {
    return b.left != 0 || !(feed_exhausted && cur >= end);
}

}  // namespace ptl
