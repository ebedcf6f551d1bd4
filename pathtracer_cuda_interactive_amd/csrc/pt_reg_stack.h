// pt_reg_stack.h — the traversal stack of trace_kernel_v2 as one 32-bit register per lane (pt_trace.h: RegStack).
//
// Small LDS-resident scenes traversed on the internal tree (left child first) need at most four stack entries, and every
// node and leaf reference of such a scene fits a signed byte.  Four bytes are one VGPR: the word replaces the lane's LDS
// stack column, its stack pointer and the column's address, and a pop no longer waits for an LDS round trip before the
// next node's address can be formed.
//
// Layout: up to four signed 8-bit references, the top of the stack in the low byte.  Every byte above the entries holds
// 0x80 (-128), which is this form's "traversal finished" value: popping the empty word yields it, again and again, the way
// the sentinel at the bottom of an LDS column does.  A push shifts the word up by a byte, so a fifth entry would lose the
// bottom one — reg_stack_on admits only trees that never hold more than four.
//
// The header needs no HIP header, so the CPU test tests/native/reg_stack_check.cpp runs the same code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_REG_HD __host__ __device__ inline
#else
#define PT_REG_HD inline
#endif

namespace ptl {

constexpr uint32_t kRegStackEmpty = 0x80808080u;
constexpr int32_t kRegStackDone = -128;
constexpr int kRegStackEntries = 4;

PT_REG_HD uint32_t reg_stack_push(uint32_t w, int32_t ref) { return (w << 8) | ((uint32_t)ref & 0xffu); }
// the top entry, sign-extended (v_bfe_i32); kRegStackDone on an empty word
PT_REG_HD int32_t reg_stack_top(uint32_t w) { return (int32_t)(int8_t)(uint8_t)(w & 0xffu); }
// the word without its top entry (v_alignbit_b32 against the constant)
PT_REG_HD uint32_t reg_stack_drop(uint32_t w) { return (w >> 8) | 0x80000000u; }

// Which launches take the register stack: scenes staged in LDS (residency 1 or 2) under their default schedule (THRESH 40,
// burst 162 — the shapes compiled with it), traversed on the internal tree in its fixed left-first order, whose tree never
// holds more than four entries (stack_need: without the sentinel) and whose references fit a byte next to the done value:
// node references 0 .. num_nodes - 1 <= 125, leaf references ~prim >= -127.
constexpr bool reg_stack_on(int res, int thresh, int inner, bool internal_tree, int stack_need, int num_nodes, int num_prims) {
    return (res == 1 || res == 2) && thresh == 40 && inner == 162 && internal_tree && stack_need <= kRegStackEntries &&
           num_nodes <= 126 && num_prims <= 127;
}

}  // namespace ptl
