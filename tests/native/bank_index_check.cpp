// Checks what the path bank carries of a work item's index (csrc/pt_path_index.h: BankIndex) against plain divisions.
//
// For every frame of the case list, every band and every chunk of the band, a simulated wave fills its bank (bank_fill),
// packs for slot s what start_path computes of item bank_item(cur, s), and hands the slots out in uneven takes (bank_take).
// What the lane of rank r receives must be the index of work item bank_item(cur, first + r) by brute force: the slot in the
// sample-major scratch buffer, and the PCG increment 2 * stream + 1 in 64 bits.  Every item of the frame must be handed out
// exactly once.  Exit code 0 = all equal.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pt_path_bank.h"
#include "pt_path_index.h"

using namespace ptl;

struct Frame {
    int width, height, spp, sample_offset, stream_stride;
    int row_begin, row_end, row_stride;
    int regions, item_order;
    uint32_t chunk;
};

// The launch constants as the host fills them in for one pass (csrc/pt_api.hip).
static RenderDev make_render_dev(const Frame& f) {
    RenderDev rd{};
    const int rows = (f.row_end - f.row_begin + f.row_stride - 1) / f.row_stride;
    rd.width = f.width; rd.height = f.height;
    rd.row_begin = f.row_begin; rd.row_step = f.row_stride; rd.num_rows = rows;
    rd.img_width = f.width;
    rd.div_img_width = make_fastdiv((uint32_t)f.width);
    rd.spp_pass = f.spp;
    rd.sample_base = f.sample_offset;
    rd.stream_stride = f.stream_stride > 0 ? f.stream_stride : f.spp;
    rd.npix = (uint32_t)rows * (uint32_t)f.width;
    rd.total_work = rd.npix * (uint32_t)f.spp;
    rd.num_regions = f.regions;
    rd.rows_per_region = (rows + f.regions - 1) / f.regions;
    rd.div_width = make_fastdiv((uint32_t)f.width);
    rd.div_spp = make_fastdiv((uint32_t)f.spp);
    rd.row_major = f.item_order;
    rd.div_npix_full = make_fastdiv((uint32_t)rd.rows_per_region * (uint32_t)f.width);
    const int full = rows / rd.rows_per_region, rest = rows - full * rd.rows_per_region;
    rd.short_region = rest ? full : -1;
    rd.div_npix_last = make_fastdiv((uint32_t)(rest > 0 ? rest : 1) * (uint32_t)f.width);
    rd.chunk = f.chunk;
    return rd;
}

// Work item `item` of `region` by plain divisions: (slot in the scratch buffer, PCG increment).
static void brute(const Frame& f, const RenderDev& rd, uint32_t region, uint32_t item, uint32_t& sample_index, uint64_t& inc) {
    const uint32_t first_row = region * (uint32_t)rd.rows_per_region;
    uint32_t rows_r = (uint32_t)rd.num_rows > first_row ? (uint32_t)rd.num_rows - first_row : 0u;
    if (rows_r > (uint32_t)rd.rows_per_region) rows_r = (uint32_t)rd.rows_per_region;
    const uint32_t w = (uint32_t)f.width;
    uint32_t s, rr, i;
    if (f.item_order) {
        i = item % w;
        const uint32_t row_s = item / w;
        rr = row_s / (uint32_t)f.spp;
        s = row_s % (uint32_t)f.spp;
    } else {
        s = item / (rows_r * w);
        const uint32_t pix = item % (rows_r * w);
        rr = pix / w;
        i = pix % w;
    }
    const uint32_t local_row = first_row + rr;
    const uint64_t j = (uint64_t)f.row_begin + (uint64_t)local_row * (uint64_t)f.row_stride;
    const uint64_t pixel = j * w + i;
    const uint64_t stream = pixel * (uint64_t)rd.stream_stride + (uint64_t)(f.sample_offset + (int)s);
    sample_index = s * rd.npix + local_row * w + i;
    inc = 2 * stream + 1;
}

static uint64_t bad = 0, checked = 0, wide = 0;

static void check_frame(const Frame& f) {
    const RenderDev rd = make_render_dev(f);
    std::vector<uint8_t> seen(rd.total_work, 0);
    uint32_t take_state = 12345u;
    for (uint32_t region = 0; region < (uint32_t)rd.num_regions; region++) {
        const uint32_t total = region_rows(rd, region) * (uint32_t)rd.width * (uint32_t)rd.spp_pass;
        for (uint32_t base = 0; base < total; base += rd.chunk) {
            uint32_t cur = base, end = base + rd.chunk < total ? base + rd.chunk : total;
            PathBank bank;
            bank_init(bank);
            while (bank_work_left(bank, true, cur, end)) {
                BankIndex slot[kBankSlots];
                if (bank.left == 0) {
                    bank_fill(bank, cur, end);
                    for (uint32_t lane = 0; lane < kBankSlots; lane++) {     // every lane packs, the slots of a short fill too
                        const PathIndex px = path_index<false>(rd, region, bank_item(cur, lane));
                        slot[lane] = bank_index_pack(px.sample_index, stream_inc(px.stream));
                    }
                }
                while (bank.left) {
                    take_state = take_state * 1664525u + 1013904223u;
                    uint32_t first;
                    const uint32_t k = bank_take(bank, 1u + (take_state >> 24) % 64u, first);
                    for (uint32_t r = 0; r < k; r++) {
                        const uint32_t item = bank_item(cur, first + r);
                        uint32_t want_w;
                        uint64_t want_inc;
                        brute(f, rd, region, item, want_w, want_inc);
                        const BankIndex& b = slot[first + r];
                        checked++;
                        wide += (want_inc >> 32) != 0;
                        if (item < base || item >= end || b.sample_index != want_w || bank_index_inc(b.inc_lo, b.inc_hi) != want_inc ||
                            want_w >= rd.total_work || seen[want_w]++) {
                            if (bad++ < 10)
                                std::printf("%dx%dx%d region %u item %u: sample_index %u want %u, inc %llx want %llx\n", f.width, f.height, f.spp,
                                            region, item, b.sample_index, want_w, (unsigned long long)bank_index_inc(b.inc_lo, b.inc_hi),
                                            (unsigned long long)want_inc);
                        }
                    }
                }
            }
        }
    }
    for (uint32_t k = 0; k < rd.total_work; k++) bad += seen[k] != 1;
}

int main() {
    const Frame shapes[] = {
        // width height spp offset stride  rows            regions order chunk
        {5, 3, 1, 0, 0, 0, 3, 1, 8, 1, 64},                 // fewer items than one bank, empty bands
        {70, 11, 3, 0, 0, 0, 11, 1, 8, 1, 64},              // width no multiple of 64, a short last band
        {24, 16, 3, 2, 0, 0, 16, 1, 8, 1, 128},             // sample_offset > 0
        {2048, 2, 2, 5, 1 << 20, 0, 2, 1, 8, 1, 64},        // streams beyond 32 bits
        {40, 31, 5, 0, 0, 1, 31, 3, 8, 1, 256},             // rows 1, 4, 7, ... : rank 1 of 3
        {640, 48, 4, 3, 1 << 20, 0, 48, 1, 1, 1, 128},      // one band
    };
    for (const Frame& s : shapes)
        for (int order = 0; order < 2; order++) {
            Frame f = s;
            f.item_order = order;
            check_frame(f);
        }
    std::printf("items %llu (increments beyond 32 bits: %llu) bad %llu\n", (unsigned long long)checked, (unsigned long long)wide,
                (unsigned long long)bad);
    return bad != 0 || wide == 0;
}
