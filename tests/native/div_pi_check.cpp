// Checks ptm::div_pi_exact's fast path (csrc/pt_math.h: div_pi_in_range / div_pi_fast, IEEE * and fma only) against
// the IEEE division x / kPi on all 2^32 fp32 bit patterns, on up to 16 threads.  Exit code 0 = bit-exact everywhere.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "pt_math.h"

static uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main() {
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<uint64_t> bad(nt, 0), fast(nt, 0);
    std::vector<uint32_t> first(nt, 0xffffffffu);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) {
        th.emplace_back([&, t] {
            const uint64_t lo = (uint64_t(1) << 32) * t / nt, hi = (uint64_t(1) << 32) * (t + 1) / nt;
            for (uint64_t b = lo; b < hi; b++) {
                float x;
                const uint32_t u = (uint32_t)b;
                std::memcpy(&x, &u, 4);
                const bool in = ptm::div_pi_in_range(x);
                const float got = in ? ptm::div_pi_fast(x) : x / ptm::kPi;
                fast[t] += in;
                if (bits_of(got) != bits_of(x / ptm::kPi)) {
                    if (!bad[t]) first[t] = u;
                    bad[t]++;
                }
            }
        });
    }
    for (auto& x : th) x.join();
    uint64_t nbad = 0, nfast = 0;
    uint32_t f = 0xffffffffu;
    for (unsigned t = 0; t < nt; t++) { nbad += bad[t]; nfast += fast[t]; if (bad[t]) f = std::min(f, first[t]); }
    std::printf("threads %u fast-path inputs %llu mismatches %llu first 0x%08x\n", nt, (unsigned long long)nfast,
                (unsigned long long)nbad, nbad ? f : 0u);
    return nbad != 0;
}
