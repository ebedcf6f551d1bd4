// pt_path_index.h — what a work item stands for: pixel, PCG stream and slot in the scratch buffer (the trace kernels of
// pt_kernels.h), and the words of it that the path bank carries per slot (pt_path_bank.h).
//
// Pure integer arithmetic on the item number and launch constants.  The header needs no HIP header, so the CPU test
// tests/native/bank_index_check.cpp runs the same code against plain divisions.
#pragma once
#include <stdint.h>

#include "pt_layout.h"

#if defined(__HIPCC__)
#define PT_PIDX_HD __host__ __device__ __forceinline__
#else
#define PT_PIDX_HD inline
#endif

namespace ptl {

PT_PIDX_HD uint32_t region_rows(const RenderDev& rp, uint32_t region) {
    const uint32_t first = region * (uint32_t)rp.rows_per_region;
    const uint32_t nrows = (uint32_t)rp.num_rows;
    const uint32_t rest = nrows - first;
    return first >= nrows ? 0u : ((uint32_t)rp.rows_per_region < rest ? (uint32_t)rp.rows_per_region : rest);
}

struct PathIndex {
    int col, j;              // image column and row
    int32_t img_width;
    uint64_t stream;         // PCG stream of the (pixel, sample)
    uint32_t sample_index;   // slot in the sample-major scratch buffer
};

// LIST: an adaptive round after the first (RenderDev::list), a compile-time variant so that plain frames keep their code.
template <bool LIST = false>
PT_PIDX_HD PathIndex path_index(const RenderDev& rp, uint32_t region, uint32_t item) {
    const uint32_t npix_r = region_rows(rp, region) * (uint32_t)rp.width;
    uint32_t s_local, rr;
    int i;
    if (rp.row_major) {
        // all samples of a row before the next row: the waves of an XCD work on a few rows of its band at a time, so the
        // primary rays (and what they hit) of one moment come from a small part of the scene
        const uint32_t row_s = fastdiv(item, rp.div_width);                    // item / width = row * spp + sample
        i = (int)(item - row_s * (uint32_t)rp.width);
        rr = fastdiv(row_s, rp.div_spp);                                       // / spp_pass
        s_local = row_s - rr * (uint32_t)rp.spp_pass;
    } else {
        s_local = fastdiv(item, (int)region == rp.short_region ? rp.div_npix_last : rp.div_npix_full);   // item / npix_r
        const uint32_t pix_r = item - s_local * npix_r;
        rr = fastdiv(pix_r, rp.div_width);                                                                // pix_r / width
        i = (int)(pix_r - rr * (uint32_t)rp.width);
    }
    const uint32_t local_row = region * (uint32_t)rp.rows_per_region + rr;
    // adaptive rounds: local_row is a position in the list of pixels still sampled (a frame of width 1, i == 0)
    uint32_t img_row = local_row;
    int col = i;
    if (LIST) {
        const uint32_t e = rp.list[local_row];
        img_row = fastdiv(e, rp.div_img_width);
        col = (int)(e - img_row * (uint32_t)rp.img_width);
    }
    const int32_t img_width = LIST ? rp.img_width : rp.width;
    const int j = rp.row_begin + (int)img_row * rp.row_step;
    const uint64_t pixel_index = (uint64_t)j * (uint64_t)img_width + (uint64_t)col;
    PathIndex px;
    px.col = col;
    px.j = j;
    px.img_width = img_width;
    px.stream = pixel_index * (uint64_t)rp.stream_stride + (uint64_t)(rp.sample_base + (int)s_local);
    px.sample_index = s_local * rp.npix + local_row * (uint32_t)rp.width + (uint32_t)i;
    return px;
}

// The PCG increment of a stream (pt_math.h: pcg_init).
PT_PIDX_HD uint64_t stream_inc(uint64_t stream) { return (stream << 1u) | 1u; }

// What a slot of the path bank carries of its item's index: the scratch-buffer slot and the PCG increment, as the 32-bit
// words of three bank registers.  bank_fill's start_path has computed both at full width; the hand-out moves the words to
// the lane that takes the path and computes nothing.  The increment is 64 bits: pixel * stream_stride passes 2^32 for
// progressive frames (stream_stride 2^20).
struct BankIndex {
    uint32_t sample_index, inc_lo, inc_hi;
};
PT_PIDX_HD BankIndex bank_index_pack(uint32_t sample_index, uint64_t inc) {
    BankIndex b;
    b.sample_index = sample_index; b.inc_lo = (uint32_t)inc; b.inc_hi = (uint32_t)(inc >> 32);
    return b;
}
PT_PIDX_HD uint64_t bank_index_inc(uint32_t inc_lo, uint32_t inc_hi) { return (uint64_t)inc_hi << 32 | inc_lo; }

}  // namespace ptl
