// pt_trace_v2_body.h — the body of trace_kernel_v2 and trace_kernel_v2_reg (pt_kernels.h), included inside each of them.
// No include guard: it is meant to be included twice.  It expects the kernel's parameters (scn, rp, lp, samples, work_counter,
// counters) and the compile-time constants RES, PRUNE, STATS, THRESH, INNER, MINW, SPEC, NEE, LIST, REG in scope.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // launch timeline (STATS builds only): 100 MHz constant clock at entry, after staging, when the wave first finds the
    // work feed dry, at exit — reduced over waves into counters[kTimelineBase..] (see flush below)
    const unsigned long long tl_entry = STATS ? wall_clock64() : 0ull;
    const ptd::SceneView sv = make_scene_view<RES>(scn, lp, smem);
    const unsigned long long tl_staged = STATS ? wall_clock64() : 0ull;
    unsigned long long tl_dry = 0;

    // LDS-resident scenes are small enough for 16-bit node / primitive references on the stack
    constexpr bool TRI_ONLY = SPEC >= 1, DIFFUSE_ONLY = SPEC >= 2;
    using STK = typename std::conditional<RES == 1 || RES == 2, int16_t, int32_t>::type;
    using STACK = typename std::conditional<REG, ptd::RegStack, ptd::LdsStack<STK>>::type;
    static_assert(!REG || ((RES == 1 || RES == 2) && THRESH == 40 && INNER == 162), "RegStack: see reg_stack_on");
    constexpr int32_t DONE = STACK::kDone;
    // INNER >= 1000 (internal tree only — exact traversal there may test leaves in ANY order): a lane that reaches a leaf sets
    // it aside (`pend`) and goes on with the next stack entry; the set-aside leaves are tested in the burst's leaf steps, when
    // many lanes have one, instead of every lane stalling on its leaf until the burst gets there.
    constexpr bool POSTPONE = INNER >= 1000;
    constexpr int BURST = INNER >= 1000 ? INNER - 1000 : INNER;
    int32_t pend = DONE;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    STACK stack;
    if constexpr (!REG) stack.col = reinterpret_cast<STK*>(smem + lp.stack_off) + (size_t)wave * scn.stack_cap * 64 + lane;

    WorkFeed feed;
    feed_init(feed, rp);
    // path bank: slot `lane` of the wave's bank = direction of the primary ray and PCG state after the two jitter draws of
    // work item bank_item(feed.cur, lane).  Where BANK_INDEX, also what start_path computed of the item's index, its slot in the
    // scratch buffer and its PCG increment (BankIndex), so that the hand-out computes nothing; elsewhere the lane that takes
    // a path works both out again from the item number (path_index)
    constexpr bool BANK = path_bank_on(RES, SPEC, NEE, LIST, THRESH, INNER);
    PathBank bank;
    bank_init(bank);
    float bank_dx = 0.0f, bank_dy = 0.0f, bank_dz = 0.0f;
    uint32_t bank_lo = 0, bank_hi = 0;
    constexpr bool BANK_INDEX = BANK && bank_index_on(REG, STATS, MINW);
    uint32_t bank_w = 0, bank_inc_lo = 0, bank_inc_hi = 0;     // BankIndex (pt_path_index.h), where BANK_INDEX
    bool alive = false;
    ptd::Ray ray;
    ray.org = ptm::mk(0, 0, 0); ray.dir = ptm::mk(0, 0, 1); ray.tnear = 0; ray.tfar = 0;
    ptd::Trav tv;
    tv.inv = ptm::mk(1, 1, 1);
    tv.best.t = 0; tv.best.u = 0; tv.best.v = 0; tv.best.prim = -1;
    tv.cur = DONE; tv.node_off = 0; tv.redo = false;
    stack.reset(tv);
    if constexpr (!REG) ptd::stack_init(stack.col);
    ptm::V3 L = ptm::mk(0, 0, 0), T = ptm::mk(1, 1, 1);
    ptm::Pcg rng;
    rng.state = 0; rng.inc = 1;
    int depth = 0;
    uint32_t my_w = 0;
    uint32_t n_paths = 0, n_segs = 0;
    ptd::TravStats st;
    st.nodes = 0; st.leaves = 0;
    // exact traversal on the internal tree (scn.fallback): rays with a zero direction component use the caller's tree and a
    // global-memory stack column of their own (the LDS columns belong to the lanes that are still traversing)
    const bool fbk = scn.fallback != 0;                       // wave-uniform
    ptd::SceneView sv_ref = sv;
    sv_ref.nodes = scn.ref_nodes; sv_ref.root_ref = scn.ref_root_ref; sv_ref.node_stride = sizeof(DNode);
    sv_ref.oct_stride = 0; sv_ref.top_nodes = nullptr; sv_ref.top_count = 0; sv_ref.fixed_order = 0;
    int32_t* redo_stk = scn.redo_stack + ((size_t)(blockIdx.x * (kBlock / 64) + wave) * (size_t)scn.redo_cap) * 64 + lane;
    uint32_t n_redo = 0;
    // next-event estimation: the lane is tracing the shadow ray of its light sample; what it resumes with afterwards
    ptd::NeeState nee;
    nee.count_emission = true; nee.want_shadow = false;
    nee.ls.wl = ptm::mk(0, 0, 1); nee.ls.tfar = 0; nee.ls.contrib = ptm::mk(0, 0, 0);
    bool in_shadow = false, cont_after = false;
    ptm::V3 next_dir = ptm::mk(0, 0, 1);

    // schedule diagnostics (STATS builds only; wave-uniform, kept in scalar registers):
    // [4] loop iterations  [5] scheduler phases  [6] lanes served by scheduler phases
    // [7] inner steps executed  [8] lanes active in them  [9] leaf steps executed  [10] lanes active in them
    // [11] lane-slots idle-waiting (finished traversal or empty) summed over traversal steps (per counter slot)
    unsigned long long dg_iter = 0, dg_sched = 0, dg_sched_lanes = 0, dg_in = 0, dg_in_lanes = 0, dg_lf = 0, dg_lf_lanes = 0, dg_wait = 0;

    for (;;) {
        const bool idle = tv.cur == DONE && (!POSTPONE || pend == DONE);
        const unsigned long long idle_mask = __ballot(idle);
        if (STATS) dg_iter++;
        // wave-uniform.  With a path bank every item the wave reserved is in [feed.cur, feed.end) or in the bank, and only this
        // wave hands out what its bank holds: work is left while either holds an item, so the loop cannot end (n_pend == 0
        // below) with path starts still banked
        const bool work_left = BANK ? bank_work_left(bank, feed.exhausted, feed.cur, feed.end) : !(feed.exhausted && feed.cur >= feed.end);
        if (STATS && !work_left && tl_dry == 0) tl_dry = wall_clock64();
        const int n_pend = __popcll(__ballot(idle && (alive || work_left)));
        // drain (no work left to refill with): fewer than THRESH lanes may be alive at all.  Scenes in global memory serve
        // the finished segments as soon as a quarter of the live lanes wait instead of waiting for the slowest traversal
        // (bunny: -1 % at 64 spp, -15 % for 2-spp frames); LDS-resident scenes gain nothing from it and keep the plain rule
        int thresh = THRESH;
        if ((RES == 0 || RES == 3) && !work_left) thresh = min(THRESH, max(1, (__popcll(__ballot(alive)) + 3) / 4));
        if (n_pend >= thresh || idle_mask == ~0ull) {
            if (n_pend == 0) break;          // every lane idle, no live path, no work left
            if (STATS) { dg_sched++; dg_sched_lanes += (unsigned)n_pend; }
            // (1) finish the segments whose traversal completed (radiance.cuh:26-75)
            if (fbk && idle && alive && tv.redo) {
                // the closest hit of this ray depends on the visit order: trace it again the reference's way, to completion
                ptd::TravStats st_redo;
                st_redo.nodes = 0; st_redo.leaves = 0;
                tv.best = ptd::intersect<false, false>(sv_ref, ray, redo_stk, st_redo);
                tv.redo = false;
                if (STATS) n_redo++;
            }
            if (idle && alive) {
                bool cont = false;
                if (NEE && in_shadow) {
                    // the shadow ray of the last bounce's light sample has been traced: add it if it arrived, then go on
                    // with the bounce that was prepared at the same time (or end the path there)
                    if (tv.best.prim < 0) L = L + nee.ls.contrib;
                    in_shadow = false;
                    cont = cont_after;
                    if (cont) { ray.dir = next_dir; ray.tnear = 1e-4f; ray.tfar = FLT_MAX; }
                } else if (tv.best.prim < 0) {
                    L = L + T * sv.bg;
                } else {
                    const ptd::Surface sf = ptd::make_surface<TRI_ONLY>(sv, ray, tv.best);
                    cont = ptd::shade_and_bounce<DIFFUSE_ONLY, NEE>(sv, sf, ray, rng, L, T, depth, rp.rr_depth, NEE ? &nee : nullptr);
                    depth++;
                    if (depth >= rp.max_depth) cont = false;
                    if (NEE && nee.want_shadow) {
                        in_shadow = true;
                        cont_after = cont;
                        next_dir = ray.dir;
                        ray.dir = nee.ls.wl; ray.tnear = 1e-4f; ray.tfar = nee.ls.tfar;     // ray.org = the hit point already
                        cont = true;
                    }
                }
                if (!cont) {
                    samples[my_w] = make_float4(L.x, L.y, L.z, 0.0f);
                    alive = false;
                }
            }
            // (2) refill dead lanes (main.cu:32-44)
            const unsigned long long need = __ballot(idle && !alive);
            if (BANK) {
                // Dead lanes take path starts out of the wave's bank; when it is empty the whole wave (the lanes that still
                // traverse included: the bank registers are theirs too) generates the next 64.  At most two rounds: what is
                // left of the bank, then a fresh one.  Lanes still without a path wait for the next phase, as they do below
                // when a chunk ends.
                unsigned long long want = need;
#pragma nounroll
                for (int round = 0; round < 2 && want; round++) {
                    if (bank.left == 0) {
                        feed_reserve(feed, rp, work_counter, lane);
                        if (feed.cur >= feed.end) break;                 // every band exhausted
                        bank_fill(bank, feed.cur, feed.end);
                        // after a short fill (the tail of a band) the first slots hold the arithmetic of items that do not
                        // exist (no memory is read for it): they are never handed out
                        const RenderDev rg = reload_render_args<STATS>();
                        const PathStart ps = start_path<LIST>(rg, feed.region, bank_item(feed.cur, (uint32_t)lane));
                        bank_dx = ps.ray.dir.x; bank_dy = ps.ray.dir.y; bank_dz = ps.ray.dir.z;
                        bank_lo = (uint32_t)ps.rng.state; bank_hi = (uint32_t)(ps.rng.state >> 32);
                        if constexpr (BANK_INDEX) {
                            const BankIndex bi = bank_index_pack(ps.sample_index, ps.rng.inc);
                            bank_w = bi.sample_index; bank_inc_lo = bi.inc_lo; bank_inc_hi = bi.inc_hi;
                        }
                    }
                    uint32_t first;
                    const uint32_t k = bank_take(bank, (uint32_t)__popcll(want), first);
                    const uint32_t rank = lane_rank(want);
                    const bool take = idle && !alive && rank < k;
                    const int src = take ? (int)(first + rank) : lane;
                    // the permutes run with every lane active (a switched-off lane gives a permute nothing to read)
                    const float dx = __shfl(bank_dx, src, 64), dy = __shfl(bank_dy, src, 64), dz = __shfl(bank_dz, src, 64);
                    const uint32_t lo = __shfl(bank_lo, src, 64), hi = __shfl(bank_hi, src, 64);
                    uint32_t w = 0, inc_lo = 0, inc_hi = 0;
                    if constexpr (BANK_INDEX) {
                        w = __shfl(bank_w, src, 64); inc_lo = __shfl(bank_inc_lo, src, 64); inc_hi = __shfl(bank_inc_hi, src, 64);
                    }
                    if (take) {
                        ray.org = ptm::mk(rp.cam_origin[0], rp.cam_origin[1], rp.cam_origin[2]);
                        ray.dir = ptm::mk(dx, dy, dz);
                        ray.tnear = 0.0f;
                        ray.tfar = __builtin_inff();
                        rng.state = (uint64_t)hi << 32 | lo;
                        if constexpr (BANK_INDEX) {
                            rng.inc = bank_index_inc(inc_lo, inc_hi);
                            my_w = w;
                        } else {
                            const PathIndex px = path_index<LIST>(rp, feed.region, bank_item(feed.cur, first + rank));
                            rng.inc = stream_inc(px.stream);
                            my_w = px.sample_index;
                        }
                        L = ptm::mk(0, 0, 0);
                        T = ptm::mk(1, 1, 1);
                        depth = 0;
                        alive = true;
                        n_paths++;
                    }
                    want = __ballot(idle && !alive);
                }
            } else if (need) {
                feed_reserve(feed, rp, work_counter, lane);
                const uint32_t avail = feed.end - feed.cur;
                if (avail) {
                    const uint32_t rank = lane_rank(need);
                    const uint32_t n = (uint32_t)__popcll(need);
                    if (idle && !alive && rank < avail) {
                        const PathStart ps = start_path<LIST>(rp, feed.region, feed.cur + rank);
                        ray = ps.ray;
                        rng = ps.rng;
                        my_w = ps.sample_index;
                        L = ptm::mk(0, 0, 0);
                        T = ptm::mk(1, 1, 1);
                        depth = 0;
                        alive = true;
                        n_paths++;
                        if (NEE) { nee.count_emission = true; in_shadow = false; }
                    }
                    feed.cur += min(n, avail);
                }
            }
            // (3) start the next traversal (scene.h:247-256)
            if (idle && alive) {
                ptd::trav_begin(sv, ray, tv, stack);
                if (!(NEE && in_shadow)) n_segs++;          // "segments" = intersect() calls; shadow rays are not counted
                // 1/d infinite on an axis: 0 * inf in the slab test is outside the argument that lets another tree stand in
                // for the caller's (pt_scene_life.hip: validate_and_build) -> straight to the reference-order rerun
                if (fbk && !(__builtin_isfinite(tv.inv.x) && __builtin_isfinite(tv.inv.y) && __builtin_isfinite(tv.inv.z))) {
                    tv.redo = true;
                    tv.cur = DONE;
                }
            }
        }
        // ---- traversal burst
        if (POSTPONE) {
            constexpr int REPS = BURST >= 100 ? BURST / 100 : 1;
            constexpr int N_IN = BURST >= 100 ? (BURST / 10) % 10 : BURST;
            constexpr int N_LF = BURST >= 100 ? BURST % 10 : 1;
#pragma unroll
            for (int r = 0; r < REPS; r++) {
#pragma unroll
                for (int k = 0; k < N_IN; k++) {
                    if (STATS) {
                        const int n_in = __popcll(__ballot(tv.cur >= 0));
                        if (n_in) { dg_in++; dg_in_lanes += (unsigned)n_in; dg_wait += (unsigned)__popcll(__ballot(tv.cur == DONE && pend == DONE)); }
                    }
                    if (tv.cur >= 0) {
                        if (STATS && !BANK) st.nodes++;
                        ptd::inner_step<PRUNE, RES == 2, (RES == 3 ? 1 : 0)>(sv, ray.org, tv, stack);
                        if (tv.cur < 0 && tv.cur != DONE && pend == DONE) {       // a leaf: set it aside, take the next entry
                            pend = tv.cur;
                            stack.pop(tv);
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < N_LF; k++) {
                    if (STATS) {
                        const int n_lf = __popcll(__ballot(pend != DONE));
                        if (n_lf) { dg_lf++; dg_lf_lanes += (unsigned)n_lf; dg_wait += (unsigned)__popcll(__ballot(tv.cur == DONE && pend == DONE)); }
                    }
                    if (pend != DONE) {
                        if (STATS && !BANK) st.leaves++;
                        ptd::leaf_test<TRI_ONLY>(sv, ray, tv, pend, fbk);
                        pend = DONE;
                        if (NEE && in_shadow && tv.best.prim >= 0) { tv.cur = DONE; stack.reset(tv); }      // occluded: done
                        if (tv.cur < 0 && tv.cur != DONE) {                       // the lane was blocked on a second leaf
                            pend = tv.cur;
                            stack.pop(tv);
                        }
                    }
                }
            }
        } else if (INNER < 0) {
            // "vote" schedule: each step runs the step kind (inner-node visit or leaf test) that more lanes wait for
#pragma unroll
            for (int k = 0; k < -INNER; k++) {
                const bool at_inner = tv.cur >= 0;
                const bool at_leaf = tv.cur < 0 && tv.cur != DONE;
                const int n_in = __popcll(__ballot(at_inner));
                const int n_lf = __popcll(__ballot(at_leaf));
                if (STATS && (n_in | n_lf)) {
                    dg_wait += (unsigned)(64 - n_in - n_lf);
                    if (n_in >= n_lf) { dg_in++; dg_in_lanes += (unsigned)n_in; } else { dg_lf++; dg_lf_lanes += (unsigned)n_lf; }
                }
                if (n_in >= n_lf) {
                    if (at_inner) {
                        if (STATS && !BANK) st.nodes++;
                        ptd::inner_step<PRUNE, RES == 2, (RES == 3 ? 1 : 0)>(sv, ray.org, tv, stack);
                    }
                } else if (at_leaf) {
                    if (STATS && !BANK) st.leaves++;
                    ptd::leaf_step<TRI_ONLY, NEE>(sv, ray, tv, stack, NEE && in_shadow, fbk);
                }
            }
        } else {
            // fixed burst: REPS x (N_IN inner steps, N_LF leaf steps).  INNER = 1..9 means (INNER, 1) x 1; INNER >= 100
            // encodes REPS*100 + N_IN*10 + N_LF (e.g. 231 = two rounds of 3 inner + 1 leaf between scheduler checks).
            constexpr int REPS = INNER >= 100 ? INNER / 100 : 1;
            constexpr int N_IN = INNER >= 100 ? (INNER / 10) % 10 : (INNER > 0 ? INNER : 1);
            constexpr int N_LF = INNER >= 100 ? INNER % 10 : 1;
#pragma unroll
            for (int r = 0; r < REPS; r++) {
#pragma unroll
                for (int k = 0; k < N_IN; k++) {
                    if (STATS) {
                        const int n_in = __popcll(__ballot(tv.cur >= 0));
                        if (n_in) { dg_in++; dg_in_lanes += (unsigned)n_in; dg_wait += (unsigned)__popcll(__ballot(tv.cur == DONE)); }
                    }
                    if (tv.cur >= 0) {
                        if (STATS && !BANK) st.nodes++;
                        ptd::inner_step<PRUNE, RES == 2, (RES == 3 ? 1 : 0)>(sv, ray.org, tv, stack);
                    }
                }
#pragma unroll
                for (int k = 0; k < N_LF; k++) {
                    if (STATS) {
                        const int n_lf = __popcll(__ballot(tv.cur < 0 && tv.cur != DONE));
                        if (n_lf) { dg_lf++; dg_lf_lanes += (unsigned)n_lf; dg_wait += (unsigned)__popcll(__ballot(tv.cur == DONE)); }
                    }
                    if (tv.cur < 0 && tv.cur != DONE) {
                        if (STATS && !BANK) st.leaves++;
                        ptd::leaf_step<TRI_ONLY, NEE>(sv, ray, tv, stack, NEE && in_shadow, fbk);
                    }
                }
            }
        }
    }
    if (BANK && STATS) {
        // the lanes active in inner and leaf steps ARE the node visits and leaf tests (every burst shape adds to dg_in_lanes /
        // dg_lf_lanes exactly the lanes that would count themselves); the bank kernels have no registers to spare for
        // per-lane copies of the two sums.  (A wave's sums fit 32 bits like a lane's: a launch has at most 2^30 work items.)
        st.nodes = lane == 0 ? (uint32_t)dg_in_lanes : 0u;
        st.leaves = lane == 0 ? (uint32_t)dg_lf_lanes : 0u;
    }
    flush_counters<STATS>(counters, lane, n_paths, n_segs, st);
    const unsigned long long redo_sum = STATS ? wave_sum(n_redo) : 0ull;
    if (STATS && lane == 0) {
        const unsigned long long tl_exit = wall_clock64();
        unsigned long long* slot = counter_slot(counters);
        atomicAdd(&slot[4], dg_iter); atomicAdd(&slot[5], dg_sched); atomicAdd(&slot[6], dg_sched_lanes);
        atomicAdd(&slot[7], dg_in); atomicAdd(&slot[8], dg_in_lanes); atomicAdd(&slot[9], dg_lf);
        atomicAdd(&slot[10], dg_lf_lanes); atomicAdd(&slot[11], dg_wait);
        atomicAdd(&slot[12], redo_sum);
        // timeline, in 10-ns ticks: [0] ~(earliest entry)  [1] latest staged  [2] ~(earliest dry)  [3] latest dry
        // [4] latest exit  [5] sum over waves of (exit - dry)  [6] sum of (dry - staged)  [7] waves
        unsigned long long* tl = counters + kTimelineBase;
        if (tl_dry == 0) tl_dry = tl_exit;
        atomicMax(&tl[0], ~tl_entry); atomicMax(&tl[1], tl_staged); atomicMax(&tl[2], ~tl_dry);
        atomicMax(&tl[3], tl_dry); atomicMax(&tl[4], tl_exit); atomicAdd(&tl[5], tl_exit - tl_dry);
        atomicAdd(&tl[6], tl_dry - tl_staged); atomicAdd(&tl[7], 1ull);
        // histograms over waves, 100-us bins after the wave's own entry: [8..135] feed found dry, [136..263] exit
        atomicAdd(&tl[8 + min(127ull, (tl_dry - tl_entry) / 10000ull)], 1ull);
        atomicAdd(&tl[136 + min(127ull, (tl_exit - tl_entry) / 10000ull)], 1ull);
    }
