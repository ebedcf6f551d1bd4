// Runs the wave-uniform bookkeeping of the path bank (csrc/pt_path_bank.h) for one wave against a simulated work feed, the
// way scheduler step (2) of trace_kernel_v2 drives it (csrc/pt_kernels.h): bands of rows with their own counters, chunks of
// 64 / 128 / 256 items, stealing from the next band, other waves taking chunks in between, and random sets of lanes whose
// paths end in a phase.  Checks, for every configuration:
//   - every item of every band is handed out exactly once (by this wave or taken by the others);
//   - a source slot is always inside the last fill, which is at most 64 slots, and below 64;
//   - bank_work_left is false only when nothing is left anywhere (feed, chunk, bank);
//   - the loop ends within 2 * items + 2 phases (every phase with a dead lane and work left hands out at least one item,
//     and every phase of the simulation ends at least one live path).
// Stand-alone; built with -fsanitize=address,undefined by tests/test_path_bank_host.py.  Exit code 0 = all held.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "pt_path_bank.h"

namespace {

struct Feed {                 // WorkFeed + feed_reserve of pt_kernels.h on plain counters
    uint32_t cur = 0, end = 0, region = 0, tried = 0;
    bool exhausted = false;
};

struct Sim {
    std::vector<uint32_t> total;       // items per band
    std::vector<uint32_t> counter;     // the band's work counter
    std::vector<std::vector<uint8_t>> given;   // [band][item] times handed out
    uint32_t chunk = 64;
    std::mt19937 rng;
    uint64_t errors = 0;

    void fail(const char* what) {
        if (errors++ < 10) std::fprintf(stderr, "FAIL: %s\n", what);
    }

    // another wave reserves a chunk of band r and traces it
    void others_take(uint32_t r) {
        const uint32_t base = counter[r];
        counter[r] += chunk;
        for (uint32_t i = base; i < base + chunk && i < total[r]; i++) given[r][i]++;
    }

    void reserve(Feed& f) {
        const uint32_t nreg = (uint32_t)total.size();
        while (f.cur >= f.end && !f.exhausted) {
            if (rng() % 4 == 0) others_take(f.region);
            const uint32_t base = counter[f.region];
            counter[f.region] += chunk;
            if (base < total[f.region]) {
                f.cur = base;
                f.end = base + chunk < total[f.region] ? base + chunk : total[f.region];
            } else if (++f.tried >= nreg) {
                f.exhausted = true;
            } else {
                f.region = (f.region + 1) % nreg;
            }
        }
    }

    bool anything_left(const Feed& f, const ptl::PathBank& b) const {
        if (b.left != 0 || f.cur < f.end) return true;
        for (size_t r = 0; r < total.size(); r++)
            if (counter[r] < total[r]) return true;
        return false;
    }

    void run(int mode) {
        uint64_t items = 0;
        for (uint32_t t : total) items += t;
        Feed feed;
        feed.region = rng() % (uint32_t)total.size();
        ptl::PathBank bank;
        ptl::bank_init(bank);
        bool alive[64] = {false};
        uint32_t filled = 0, filled_region = 0;      // slots and band of the last fill
        const uint64_t bound = 2 * items + 2;
        uint64_t phases = 0;
        for (;; phases++) {
            if (phases > bound) { fail("loop did not end within the bound"); return; }
            const bool work_left = ptl::bank_work_left(bank, feed.exhausted, feed.cur, feed.end);
            // the feed is exhausted only after every band was found empty, so before that work_left must hold
            if (!work_left && anything_left(feed, bank)) { fail("work_left false with items left"); return; }
            int n_pend = 0;
            for (int l = 0; l < 64; l++) n_pend += alive[l] || work_left;
            if (n_pend == 0) break;
            // (1) some live paths end: all of them, one, or a random set
            int live[64], n_live = 0;
            for (int l = 0; l < 64; l++) if (alive[l]) live[n_live++] = l;
            if (n_live) {
                const int m = mode == 0 ? (int)(rng() % 3) : mode - 1;
                if (m == 0) for (int k = 0; k < n_live; k++) alive[live[k]] = false;
                else if (m == 1) alive[live[rng() % (uint32_t)n_live]] = false;
                else {
                    bool any = false;
                    for (int k = 0; k < n_live; k++) if (rng() % 3 == 0) { alive[live[k]] = false; any = true; }
                    if (!any) alive[live[0]] = false;
                }
            }
            // (2) hand out: at most two rounds
            for (int round = 0; round < 2; round++) {
                uint32_t n_need = 0;
                for (int l = 0; l < 64; l++) n_need += !alive[l];
                if (!n_need) break;
                if (bank.left == 0) {
                    reserve(feed);
                    if (feed.cur >= feed.end) break;
                    const uint32_t before = feed.cur;
                    filled = ptl::bank_fill(bank, feed.cur, feed.end);
                    filled_region = feed.region;
                    if (filled == 0 || filled > ptl::kBankSlots || bank.left != filled || feed.cur != before + filled ||
                        feed.cur > feed.end || ptl::bank_item(feed.cur, ptl::kBankSlots - filled) != before)
                        fail("bank_fill");
                }
                // nothing may have moved the feed to another band or chunk while the bank held items
                if (feed.region != filled_region) { fail("the feed changed its band under a filled bank"); return; }
                uint32_t first = 0;
                const uint32_t k = ptl::bank_take(bank, n_need, first);
                if (k == 0) fail("a round with slots left handed out nothing");
                uint32_t rank = 0;
                for (int l = 0; l < 64; l++) {
                    if (alive[l]) continue;
                    if (rank < k) {
                        const uint32_t slot = first + rank;
                        if (!(slot < ptl::kBankSlots && slot >= ptl::kBankSlots - filled)) { fail("source slot out of range"); return; }
                        const uint32_t item = ptl::bank_item(feed.cur, slot);
                        if (item >= total[feed.region]) { fail("item past its band"); return; }
                        given[feed.region][item]++;
                        alive[l] = true;
                    }
                    rank++;
                }
            }
        }
        for (size_t r = 0; r < total.size(); r++)
            for (uint32_t i = 0; i < total[r]; i++)
                if (given[r][i] != 1) { fail("an item was not handed out exactly once"); return; }
    }
};

}  // namespace

int main() {
    std::mt19937 top(20251);
    const uint32_t fixed_sizes[] = {0, 1, 15, 63, 64, 65, 127, 128, 144, 191, 256, 257, 1000};
    uint64_t runs = 0, errors = 0;
    for (int rep = 0; rep < 3000; rep++) {
        Sim s;
        s.rng.seed(top());
        const uint32_t nbands = 1 + top() % 8;
        s.chunk = 64u << (top() % 3);
        for (uint32_t r = 0; r < nbands; r++) {
            const uint32_t pick = top() % 4;
            const uint32_t t = pick == 0 ? 0u : pick == 1 ? fixed_sizes[top() % (sizeof fixed_sizes / sizeof fixed_sizes[0])] : top() % 3000;
            s.total.push_back(t);
            s.counter.push_back(0);
            s.given.emplace_back(t, (uint8_t)0);
        }
        s.run(rep % 4);
        runs++;
        errors += s.errors;
    }
    std::printf("runs %llu errors %llu\n", (unsigned long long)runs, (unsigned long long)errors);
    return errors != 0;
}
