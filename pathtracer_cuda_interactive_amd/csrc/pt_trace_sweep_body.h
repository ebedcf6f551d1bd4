// pt_trace_sweep_body.h — the body of trace_kernel_v2_sweep (pt_kernels.h), included inside it.
// The schedule of trace_kernel_v2 (scheduler phase at THRESH lanes, path bank) around a traversal without a tree
// (pt_leaf_sweep.h, pt_sweep_layout.h): step (3) of the phase tests every distinct leaf box of the scene against the new segment
// and leaves the lane one hit bit per group; the burst is leaf tests alone, group by group, each group's primitives along the
// chain of its slot records.  No inner step, no stack, and 1/d is dead once the phase ends.  The block stages the sweep's own
// tables (box tables, slot records, skip entries) where the tree kernel stages the 8 octant node tables: the tree is never walked here, and
// a rerun reads the caller's tree in global memory.  The launches that take it: leaf_sweep_on — residency 2, exact traversal
// on the internal tree (so scn.fallback is set: ties on t are settled in the caller's visit order and a ray with a non-finite
// 1/d is traced on the caller's tree), triangles with diffuse materials, no counting, no next-event estimation, no pixel list.
// It expects the kernel's parameters (scn, rp, lp, samples, work_counter, counters, sweep) and MINW, N_LEAF in scope.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int THRESH = PT_SWEEP_THRESH;
    typedef const __attribute__((address_space(3))) unsigned char* LdsBytes;
    typedef float f2v __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(3))) f2v* LdsF2;
    const uint32_t n_groups = sweep.groups;                        // 1 .. kSweepMaxBoxes
    const uint32_t box_pitch = sweep.box_pitch;
    const uint64_t cls_bits = __builtin_bit_cast(uint64_t, sweep.classes);    // the sweep loops' trip counts, a byte each, in two scalars
    const ptd::SceneView sv = make_sweep_view(scn, lp, sweep, smem);
    const ptd::lds_f4v* slots = (const ptd::lds_f4v*)(smem + lp.nodes_off + sweep_slots_off(n_groups));

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;

    WorkFeed feed;
    feed_init(feed, rp);
    PathBank bank;
    bank_init(bank);
    float bank_dx = 0.0f, bank_dy = 0.0f, bank_dz = 0.0f;
    uint32_t bank_lo = 0, bank_hi = 0;
    uint32_t bank_w = 0, bank_inc_lo = 0, bank_inc_hi = 0;     // BankIndex (pt_path_index.h)
    bool alive = false;
    ptd::Ray ray;
    ray.org = ptm::mk(0, 0, 0); ray.dir = ptm::mk(0, 0, 1); ray.tnear = 0; ray.tfar = 0;
    ptd::Trav tv;                                  // best and redo alone are live: no node, no stack, no 1/d
    tv.inv = ptm::mk(1, 1, 1);
    tv.best.t = 0; tv.best.u = 0; tv.best.v = 0; tv.best.prim = -1;
    tv.cur = 0; tv.stack_state = 0; tv.node_off = 0; tv.redo = false;
    uint32_t hits = 0;                             // groups whose box this segment hits and that are not yet taken up: group k = bit 31 - k
                                                   // (between steps (1) and (3) of a phase: the groups a bounce need not test)
    uint32_t pend = 0;                             // the slot to test next inside the group taken up last, 0 = none
    ptm::V3 L = ptm::mk(0, 0, 0), T = ptm::mk(1, 1, 1);
    ptm::Pcg rng;
    rng.state = 0; rng.inc = 1;
    int depth = 0;
    uint32_t my_w = 0;
    uint32_t n_paths = 0, n_segs = 0;              // of the wave (scalar registers: a phase has no vector register to spare)
    ptd::TravStats st;
    st.nodes = 0; st.leaves = 0;
    ptd::SceneView sv_ref = sv;
    sv_ref.nodes = scn.ref_nodes; sv_ref.root_ref = scn.ref_root_ref; sv_ref.node_stride = sizeof(DNode);
    sv_ref.oct_stride = 0; sv_ref.top_nodes = nullptr; sv_ref.top_count = 0; sv_ref.fixed_order = 0;
    int32_t* redo_stk = scn.redo_stack + ((size_t)(blockIdx.x * (kBlock / 64) + wave) * (size_t)scn.redo_cap) * 64 + lane;

    for (;;) {
        const bool idle = (hits | pend) == 0u;
        const unsigned long long idle_mask = __ballot(idle);
        const bool work_left = bank_work_left(bank, feed.exhausted, feed.cur, feed.end);
        const int n_pend = __popcll(__ballot(idle && (alive || work_left)));
        if (n_pend >= THRESH || idle_mask == ~0ull) {
            if (n_pend == 0) break;          // every lane idle, no live path, no work left
            // (1) finish the segments whose candidates are used up (radiance.cuh:26-75)
            if (idle && alive && tv.redo) {
                // 1/d is not finite: trace this ray the reference's way on the caller's tree, to completion.  tfar is not kept
                // across the burst (the leaf tests here do not read it): a path's first segment is the camera's.
                ptd::TravStats st_redo;
                st_redo.nodes = 0; st_redo.leaves = 0;
                ray.tfar = depth == 0 ? __builtin_inff() : FLT_MAX;
                tv.best = ptd::intersect<false, false>(sv_ref, ray, redo_stk, st_redo);
                tv.redo = false;
            }
            if (idle && alive) {
                bool cont = false;
                if (tv.best.prim < 0) {
                    L = L + T * sv.bg;
                } else {
                    const ptd::Surface sf = ptd::make_surface<true>(sv, ray, tv.best);
                    cont = ptd::shade_and_bounce<true, false>(sv, sf, ray, rng, L, T, depth, rp.rr_depth, nullptr);
                    depth++;
                    if (depth >= rp.max_depth) cont = false;
                }
                if (!cont) {
                    samples[my_w] = make_float4(L.x, L.y, L.z, 0.0f);
                    alive = false;
                } else {
                    // The bounce starts on the primitive it hit.  Where that primitive's group is flat on an axis and the new
                    // origin lies on its plane bit for bit, no triangle of that plane can be kept as a hit of the next segment
                    // (pt_sweep_skip.h has the argument): step (3) takes those groups out of the hit word.  `hits` is zero in
                    // an idle lane and the sweep accumulates in h, so the skip word waits there; a lane that does not go on
                    // keeps its zero, a refilled lane (camera ray) never comes by here.
                    typedef const __attribute__((address_space(3))) uint32_t* LdsWords;
                    LdsWords e = (LdsWords)((LdsBytes)smem + lp.nodes_off + sweep_skip_off(n_groups, (uint32_t)scn.num_prims) +
                                            (uint32_t)tv.best.prim * (uint32_t)sizeof(SweepSkipEntry));
                    const float skip_c = __builtin_bit_cast(float, e[0]);
                    const uint32_t skip_mask = e[1], skip_axis = e[2];
                    const float oa = skip_axis == 0u ? ray.org.x : skip_axis == 1u ? ray.org.y : ray.org.z;
                    hits = oa == skip_c ? skip_mask : 0u;
                }
            }
            // (2) refill dead lanes out of the wave's path bank (pt_trace_v2_body.h has the account of it)
            unsigned long long want = __ballot(idle && !alive);
#pragma nounroll
            for (int round = 0; round < 2 && want; round++) {
                if (bank.left == 0) {
                    feed_reserve(feed, rp, work_counter, lane);
                    if (feed.cur >= feed.end) break;                 // every band exhausted
                    bank_fill(bank, feed.cur, feed.end);
                    const RenderDev rg = reload_render_args<false>();
                    const PathStart ps = start_path<false>(rg, feed.region, bank_item(feed.cur, (uint32_t)lane));
                    bank_dx = ps.ray.dir.x; bank_dy = ps.ray.dir.y; bank_dz = ps.ray.dir.z;
                    bank_lo = (uint32_t)ps.rng.state; bank_hi = (uint32_t)(ps.rng.state >> 32);
                    const BankIndex bi = bank_index_pack(ps.sample_index, ps.rng.inc);
                    bank_w = bi.sample_index; bank_inc_lo = bi.inc_lo; bank_inc_hi = bi.inc_hi;
                }
                uint32_t first;
                const uint32_t k = bank_take(bank, (uint32_t)__popcll(want), first);
                const uint32_t rank = lane_rank(want);
                const bool take = idle && !alive && rank < k;
                const int src = take ? (int)(first + rank) : lane;
                const float dx = __shfl(bank_dx, src, 64), dy = __shfl(bank_dy, src, 64), dz = __shfl(bank_dz, src, 64);
                const uint32_t lo = __shfl(bank_lo, src, 64), hi = __shfl(bank_hi, src, 64);
                const uint32_t w = __shfl(bank_w, src, 64), inc_lo = __shfl(bank_inc_lo, src, 64), inc_hi = __shfl(bank_inc_hi, src, 64);
                if (take) {
                    ray.org = ptm::mk(rp.cam_origin[0], rp.cam_origin[1], rp.cam_origin[2]);
                    ray.dir = ptm::mk(dx, dy, dz);
                    ray.tnear = 0.0f;
                    rng.state = (uint64_t)hi << 32 | lo;
                    rng.inc = bank_index_inc(inc_lo, inc_hi);
                    my_w = w;
                    L = ptm::mk(0, 0, 0);
                    T = ptm::mk(1, 1, 1);
                    depth = 0;
                    alive = true;
                }
                n_paths += k;
                want = __ballot(idle && !alive);
            }
            // (3) start the next segment (scene.h:247-256): the box sweep
            n_segs += (uint32_t)__popcll(__ballot(idle && alive));
            if (idle && alive) {
                // The record stream (pt_kernels.h: SweepWindow) starts here, in front of the reciprocals: the lane's octant is the
                // sign bits of d — a lane that sweeps has a finite 1/d, whose sign is d's; a lane that does not takes the rerun
                // and never reads h, and every octant's table is inside the staged region — so the first record's four pairs
                // and the PAIR2 counts (one scalar load of the kernel's arguments, a word for four classes; they hold no scalar
                // register outside this step) are under way while the three reciprocals are formed.  One wait behind them takes
                // both: no scalar load is outstanding while the stream runs, so its waits can count LDS reads in order.
                const uint32_t oct = (__builtin_bit_cast(uint32_t, ray.dir.x) >> 31) | ((__builtin_bit_cast(uint32_t, ray.dir.y) >> 31) << 1) |
                                     ((__builtin_bit_cast(uint32_t, ray.dir.z) >> 31) << 2);
                LdsF2 bx = (LdsF2)((LdsBytes)smem + lp.nodes_off + oct * box_pitch);
                SweepWindow win;
                bx = sweep_window_read(win, bx, 0);
                typedef uint32_t FamWords __attribute__((ext_vector_type(4), aligned(4)));
                typedef const volatile __attribute__((address_space(4))) FamWords* KernargFamWords;
                KernargFamWords fw = (KernargFamWords)((const __attribute__((address_space(4))) unsigned char*)__builtin_amdgcn_kernarg_segment_ptr() +
                                                       offsetof(SweepKernelArgs, sweep) + offsetof(SweepLayoutDev, fam));
                asm volatile("" : "+s"(fw));
                const FamWords fam = *fw;                              // three words and the struct's padding
                uint32_t f0 = fam.x, f1 = fam.y, f2 = fam.z;
                __builtin_amdgcn_sched_barrier(0);
                const ptm::V3 inv = ptm::mk(ptm::rcp_exact(ray.dir.x), ptm::rcp_exact(ray.dir.y), ptm::rcp_exact(ray.dir.z));
                asm volatile("" : "+s"(f0), "+s"(f1), "+s"(f2));
                tv.best.t = FLT_MAX; tv.best.u = 0.0f; tv.best.v = 0.0f; tv.best.prim = -1;
                // 1/d infinite on an axis: 0 * inf in the slab test is outside the argument that lets the leaf boxes alone decide
                // (pt_scene_life.hip: validate_and_build) -> the reference-order rerun in the next phase, no candidates
                tv.redo = !(__builtin_isfinite(inv.x) && __builtin_isfinite(inv.y) && __builtin_isfinite(inv.z));
                if (!tv.redo) {
                    // the lane's octant box table, in LDS's 32-bit address space, read front to back through the window: two
                    // groups per record, no table of offsets or masks, one hit bit per group shifted in (hits = 2 * hits + hit)
                    const ptm::V3 o = ray.org;
                    // h = 2 * h + hit as the compare and ONE add-with-carry, h + h + the compare's lane mask, where the compiler's
                    // own choice is a select per group and a shift and an or per pair (2.5 per group on top of the compare).
                    // gfx950 wants two wait states between a vector instruction that writes a lane mask and one that reads it,
                    // and nothing inserts them inside an asm statement: a pair interleaves its two compares and adds and needs
                    // one s_nop, the odd group alone waits two.
                    uint32_t h = 0;
                    // the pairs that share an axis interval come first, class by class (pt_sweep_pairs.h): the shared axis's
                    // products once per pair, records of 10 floats; a class the scene does not have costs its scalar branch.
                    // The counts are taken out of their two words HERE, by scalar instructions: the empty statement keeps the
                    // compiler from holding eight counts and eight "is zero" masks in scalar registers across the main loop,
                    // which it has not got (they overflowed into the lanes of a vector register, one more than the kernel has).
                    uint32_t cls_lo = (uint32_t)cls_bits, cls_hi = (uint32_t)(cls_bits >> 32);
                    asm volatile("" : "+s"(cls_lo), "+s"(cls_hi));
                    SweepPairClasses cls;
                    cls.flat[0] = (uint8_t)cls_lo; cls.flat[1] = (uint8_t)(cls_lo >> 8); cls.flat[2] = (uint8_t)(cls_lo >> 16);
                    cls.share[0] = (uint8_t)(cls_lo >> 24); cls.share[1] = (uint8_t)cls_hi; cls.share[2] = (uint8_t)(cls_hi >> 8);
                    cls.general = (uint8_t)(cls_hi >> 16); cls.single = (uint8_t)(cls_hi >> 24);
                    // the PAIR2 records in front of them (pt_sweep_families.h); a word of zeros is one branch
                    if (f0) {
                        bx = sweep_pair2<0, false, false>(bx, win, f0 & 0xffu, o, inv, h);
                        bx = sweep_pair2<0, true, false>(bx, win, (f0 >> 8) & 0xffu, o, inv, h);
                        bx = sweep_pair2<0, false, true>(bx, win, (f0 >> 16) & 0xffu, o, inv, h);
                        bx = sweep_pair2<0, true, true>(bx, win, f0 >> 24, o, inv, h);
                    }
                    if (f1) {
                        bx = sweep_pair2<1, false, false>(bx, win, f1 & 0xffu, o, inv, h);
                        bx = sweep_pair2<1, true, false>(bx, win, (f1 >> 8) & 0xffu, o, inv, h);
                        bx = sweep_pair2<1, false, true>(bx, win, (f1 >> 16) & 0xffu, o, inv, h);
                        bx = sweep_pair2<1, true, true>(bx, win, f1 >> 24, o, inv, h);
                    }
                    if (f2) {
                        bx = sweep_pair2<2, false, false>(bx, win, f2 & 0xffu, o, inv, h);
                        bx = sweep_pair2<2, true, false>(bx, win, (f2 >> 8) & 0xffu, o, inv, h);
                        bx = sweep_pair2<2, false, true>(bx, win, (f2 >> 16) & 0xffu, o, inv, h);
                        bx = sweep_pair2<2, true, true>(bx, win, f2 >> 24, o, inv, h);
                    }
                    bx = sweep_shared_pairs<0, true>(bx, win, cls.flat[0], o, inv, h);
                    bx = sweep_shared_pairs<1, true>(bx, win, cls.flat[1], o, inv, h);
                    bx = sweep_shared_pairs<2, true>(bx, win, cls.flat[2], o, inv, h);
                    bx = sweep_shared_pairs<0, false>(bx, win, cls.share[0], o, inv, h);
                    bx = sweep_shared_pairs<1, false>(bx, win, cls.share[1], o, inv, h);
                    bx = sweep_shared_pairs<2, false>(bx, win, cls.share[2], o, inv, h);
                    // the general pair, visit_node<false, true>: the same operations on the same operands (near.xy | near.z far.x |
                    // far.yz per box); the window is box A and B's near.xy, the tail the rest of B
                    // (the loop vectoriser would pair the groups up into packed fp32, which issues at half rate)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
                    for (uint32_t k = cls.general; k != 0; k--) {
                        const f2v b1 = bx[4], b2 = bx[5];
                        __builtin_amdgcn_sched_barrier(0);
                        const float d_anx = win.p0.x - o.x, d_any = win.p0.y - o.y, d_anz = win.p1.x - o.z;
                        const float d_afx = win.p1.y - o.x, d_afy = win.p2.x - o.y, d_afz = win.p2.y - o.z;
                        const float d_bnx = win.p3.x - o.x, d_bny = win.p3.y - o.y, d_bnz = b1.x - o.z;
                        const float d_bfx = b1.y - o.x, d_bfy = b2.x - o.y, d_bfz = b2.y - o.z;
                        bx = sweep_window_read(win, bx, 6);
                        const float tna = ptm::fmax2(0.0f, ptm::fmax2(ptm::fmax2(d_anx * inv.x, d_any * inv.y), d_anz * inv.z));
                        const float tfa = ptm::fmin2(ptm::fmin2(d_afx * inv.x, d_afy * inv.y), d_afz * inv.z);
                        const float tnb = ptm::fmax2(0.0f, ptm::fmax2(ptm::fmax2(d_bnx * inv.x, d_bny * inv.y), d_bnz * inv.z));
                        const float tfb = ptm::fmin2(ptm::fmin2(d_bfx * inv.x, d_bfy * inv.y), d_bfz * inv.z);
                        sweep_shift_in_two(h, tfa, tna, tfb, tnb);
                    }
                    if (cls.single) {                                             // an odd count: the last group alone, three pairs of the window
                        const float tn = ptm::fmax2(ptm::fmax2((win.p0.x - o.x) * inv.x, (win.p0.y - o.y) * inv.y), (win.p1.x - o.z) * inv.z);
                        const float tf = ptm::fmin2(ptm::fmin2((win.p1.y - o.x) * inv.x, (win.p2.x - o.y) * inv.y), (win.p2.y - o.z) * inv.z);
                        const float tn0 = ptm::fmax2(0.0f, tn);
                        asm("v_cmp_ge_f32_e32 vcc, %1, %2\n\ts_nop 1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(h) : "v"(tf), "v"(tn0) : "vcc");
                    }
                    hits = sweep_hits_align(h, n_groups) & ~hits;         // without the groups of the plane a bounce starts on (step (1))
                } else {
                    hits = 0u;                                            // the rerun takes every leaf: the skip word goes unused
                }
            }
        }
        // ---- burst: N_LEAF leaf tests.  A lane goes on inside the group it took up last (pend: the link of the record just
        // tested), else it takes up the first group whose hit bit is set: groups in table order, a group's primitives in ascending
        // order.  That is not the order of the tree kernel, and need not be: exact traversal on the internal tree may test the
        // leaves in ANY order (pt_scene_life.hip: validate_and_build) — the set of leaves tested is the set whose box the ray hits,
        // the closest hit is the minimum over that set, and where two of them tie on t the leaf test asks the caller's tree
        // which one the reference visits first (ref_visits_first), a question of the two primitives alone, not of which was
        // tested first.
#pragma unroll
        for (int k = 0; k < N_LEAF; k++) {
            if ((hits | pend) != 0u) {
                uint32_t slot = pend;
                if (pend == 0u) {
                    slot = sweep_first_group(hits);
                    hits = sweep_clear_group(hits, slot);
                }
                pend = ptd::leaf_test_slot(sv, slots, ray, tv, slot);
            }
        }
    }
    flush_counters<false>(counters, lane, lane == 0 ? n_paths : 0u, lane == 0 ? n_segs : 0u, st);
