// ocean_launch.h -- launch_frame<N>: the launches of one frame at tile size N, three at most (included by frames_*.hip).
#pragma once
#include <cstdlib>

#include "ocean_ctx.h"

using namespace ocean;

// ---------------------------------------------------------------------------------
template <class K>
static hipError_t allow_lds(K kernel, size_t bytes)
{
    if (bytes <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes);
}

// One kernel launch.  With an event pair the launch goes through hipExtLaunchKernelGGL, which attaches the events
// to the dispatch itself: their interval is the kernel's own execution time (what rocprofv3 reports), free of the
// 2.5-3 us of marker/launch processing that events recorded around a launch carry.
template <class K, class... A>
static void launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, hipEvent_t* ev, A... args)
{
    if (ev) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, st, ev[0], ev[1], 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}

// tile sizes whose single-tile frames run the merged x pass (measured: profiles/r05_small_tile_experiments.txt); alone = a serial frame
template <int N> constexpr bool xmerge_pays(bool alone) { return alone ? N <= 128 : N <= 512; }

template <int N>
static hipError_t launch_frame(ocean_ctx* c, const FrameArgs& a, FrameLaunch& fl)
{
    const FramePolicy& p = fl.policy;
    const hipStream_t st = fl.stream;
    using G = Geo<N>;
    using HF = Half<N>;
    const unsigned tiles = c->tiles;
    hipError_t e;
    constexpr int C = G::CC;
    constexpr size_t lds_rows = zpass_lds_bytes<N, 1>();
    constexpr bool HAS2 = zpass_has_width2<N>();
    constexpr size_t lds_rows2 = zpass_lds_bytes<N, 2>();
    constexpr size_t lds_m = xpass_disp_lds_bytes<N, C, G::T_C, typename G::PC>(), lds_b = xpass_b_lds_bytes<N, C, G::T_C, typename G::PC>();
    static_assert(lds_b <= 80 * 1024, "two x-pass workgroups per compute unit");
    static_assert(HF::NUP % (2 * C) == 0, "height row blocks");
    constexpr unsigned hb_b = xpass_height_groups<N, C>(), nb = xpass_row_groups<N, C>(), xg = xpass_merged_groups<N, C>();
    const bool fast = !a.h0h && a.omega_q;       // the usual form of the spectrum: fp32 h0, 16-bit dispersion
    const bool alone = p.alone;
    const unsigned cus = (unsigned)(c->cu_count > 0 ? c->cu_count : 0);
    // Staggered start (ocean_kernels.h: start_ramp_wait; the rule and its constants: OceanTuning, ocean_ctx.h).  A launch gets one when its WHOLE
    // grid is resident at once on this device -- grid <= compute units x resident workgroups per unit, the latter asked of the runtime for the
    // kernels in question -- and it covers enough texels for the bursts to be worth separating; the spread is a fraction of its expected duration.
    // In practice: the three launches of one 2048^2 tile (every mode and precision), 4.2 / 5.1 / 4.0 us serial, the x passes twice that when
    // pipelined; not 1024^2 (too few texels), not 4096^2 or batches (several rounds, which overlap by themselves).  ocean_set_start_ramp(ctx, 0)
    // switches it off altogether (a device shared with other work: a workgroup's wait is simply lost).
    int ramp_z = 0, ramp_b = 0, ramp_d = 0;          // (computed below, once the kernels' attributes are set)
    // function attributes are per device; a context belongs to one device and one thread, so the flag
    // lives in the context (no process-wide state shared between contexts or threads)
    // Which forms of the z pass a tile size has (ocean_kernels.h).  ZW1: one column, two-transform batches (four-transform batches at 256 /
    // 512) -- every size below 1024 and a single 1024^2 tile; C1: one column, single-transform batches, half the threads -- 4096^2
    // always, 2048^2 and batches of 1024^2 unless the intermediates are streamed; ZW2: two neighbouring columns (whole-line stores) --
    // streamed intermediates at 1024^2 and 2048^2.  Developer builds keep every form for A/B runs (OCEAN_ZW, OCEAN_ZC1).
#ifdef OCEAN_DEVELOPER
    constexpr bool DEV = true;
#else
    constexpr bool DEV = false;
#endif
    constexpr bool HAS1 = DEV || N <= 1024;
    constexpr bool HASC1 = zpass_has_c1<N>();
    constexpr bool HAS2_PLAIN = DEV && HAS2;              // (the two-column form with plain stores: never selected by the shipped rules)
    if (c->attr_n != (uint32_t)N) {
#define OCEAN_ALLOW_Z(znt, z16, fast) \
        if constexpr (HAS1) if ((e = allow_lds(k_zpass<N, G::T_ROWS, typename G::PR, znt, z16, 1, fast>, lds_rows)) != hipSuccess) return e; \
        if constexpr (HAS2 && (znt || HAS2_PLAIN)) if ((e = allow_lds(k_zpass<N, G::T_ROWS, typename G::PR, znt, z16, 2, fast>, lds_rows2)) != hipSuccess) return e; \
        if constexpr (HASC1) if ((e = allow_lds(k_zpass_c1<N, zpass_c1_threads<N>(), typename C1Plan<N>::type, znt, z16, fast>, zpass_c1_lds_bytes<N>())) != hipSuccess) return e; \
        if constexpr (HASC1 && zpass_has_wt<N>() && !znt && !z16) if ((e = allow_lds(k_zpass_c1<N, zpass_c1_threads<N>(), typename C1Plan<N>::type, false, false, fast, true>, zpass_c1_lds_bytes<N>())) != hipSuccess) return e;
#define OCEAN_ALLOW_Z2(fast) OCEAN_ALLOW_Z(false, false, fast) OCEAN_ALLOW_Z(true, false, fast) OCEAN_ALLOW_Z(false, true, fast) OCEAN_ALLOW_Z(true, true, fast)
        OCEAN_ALLOW_Z2(true) OCEAN_ALLOW_Z2(false)
#undef OCEAN_ALLOW_Z2
#undef OCEAN_ALLOW_Z
#define OCEAN_ALLOW_X1(kern, lds, z16, jac) \
        if ((e = allow_lds(kern<N, C, G::T_C, typename G::PC, false, z16, jac>, lds)) != hipSuccess) return e; \
        if ((e = allow_lds(kern<N, C, G::T_C, typename G::PC, true, z16, jac>, lds)) != hipSuccess) return e;
#define OCEAN_ALLOW_X2(kern, lds, jac) OCEAN_ALLOW_X1(kern, lds, false, jac) OCEAN_ALLOW_X1(kern, lds, true, jac)
#define OCEAN_ALLOW_X(kern, lds) OCEAN_ALLOW_X2(kern, lds, false) OCEAN_ALLOW_X2(kern, lds, true)
        OCEAN_ALLOW_X(k_xpass_b, lds_b)
        OCEAN_ALLOW_X(k_xpass_disp, lds_m)
#undef OCEAN_ALLOW_X
#undef OCEAN_ALLOW_X2
#undef OCEAN_ALLOW_X1
        c->attr_n = (uint32_t)N;
    }
    if (c->start_ramp && cus) {
        if (c->occ_n != N) {
            int oz = 0, oza = 0, ob = 0, od = 0;
            if constexpr (zpass_has_c1<N>()) {      // (the usual form of the spectrum and the instantiation that carries every form: different launch bounds)
                (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&oz, k_zpass_c1<N, zpass_c1_threads<N>(), typename C1Plan<N>::type, false, false, true>,
                                                                   zpass_c1_threads<N>(), zpass_c1_lds_bytes<N>());
                (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&oza, k_zpass_c1<N, zpass_c1_threads<N>(), typename C1Plan<N>::type, false, false, false>,
                                                                   zpass_c1_threads<N>(), zpass_c1_lds_bytes<N>());
            }
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&ob, k_xpass_b<N, C, G::T_C, typename G::PC, false, false, false>, G::T_C, lds_b);
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&od, k_xpass_disp<N, C, G::T_C, typename G::PC, false, false, false>, G::T_C, lds_m);
            (void)hipGetLastError();
            c->occ_z = oz; c->occ_z_all = oza; c->occ_b = ob; c->occ_d = od; c->occ_n = N;
        }
        int bpt[3];
        ocean_launch_bytes_per_texel(p.half_inter, a.mode == 3, a.h0h != nullptr, a.omega_q != nullptr, bpt);
        const OceanTuning& tu = c->tune;
        const double texels = (double)tiles * N * N;
        auto ramp_ticks = [&](int bytes_per_texel, unsigned workgroups, int per_cu, double scale) -> int {
            const double bytes = texels * bytes_per_texel;
            const unsigned slots = (unsigned)per_cu < tu.ramp_max_wg_per_cu ? (unsigned)per_cu : tu.ramp_max_wg_per_cu;
            if (per_cu <= 0 || workgroups > slots * cus || texels < tu.ramp_min_texels) return 0;
            return (int)(tu.ramp_frac * scale * bytes / tu.ramp_rate_bytes_per_s * 1.0e8 + 0.5);      // 10 ns ticks (s_memrealtime)
        };
        ramp_z = ramp_ticks(bpt[0], (unsigned)(N / 2 + 1) * tiles, fast ? c->occ_z : c->occ_z_all, 1.0);
        // k_xpass_b: over its NORMAL workgroups and their bytes alone -- the height workgroups (2 B/texel in, 2 out) write next to nothing and all
        // start at once (item 10); the Jacobian mode's few workgroups beyond one round do not change the picture (item 12: same gain)
        ramp_b = ramp_ticks(bpt[1] - 4, (hb_b + nb) * tiles, c->occ_b, alone ? 1.0 : tu.ramp_pipelined_x);
        ramp_d = ramp_ticks(bpt[2], nb * tiles, c->occ_d, alone ? 1.0 : tu.ramp_pipelined_x);
    }
    // the form of the z pass (see above); the usual form of the spectrum (fp32 h0, 16-bit dispersion) has instantiations without the
    // other forms' code (FAST)
    bool c1 = HASC1 && zpass_c1_pays<N>(p.nt_inter, tiles);
    bool zw2 = HAS2 && !c1 && p.nt_inter;
    // a SERIAL frame's fp32 intermediates go out write-through where that form exists (ocean_kernels.h: store_z, zpass_has_wt)
    constexpr bool HAS_WT = HASC1 && zpass_has_wt<N>();
    const bool wt_frame = HAS_WT && alone && !p.nt_inter && !p.half_inter && c->z_write_through;
    bool z_wt = c1 && wt_frame;
    // Frame order: z pass (four transforms per column) -> k_xpass_b (HEIGHT + NORMAL workgroups) -> k_xpass_disp.  (Round 5 also ran a SPLIT
    // order -- z pass {height, pair 0} -> HEIGHT workgroups -> k_xpass_disp -> z pass {pair 1, pair 2} -> NORMAL workgroups: bit-identical, slower
    // at every size -- the x passes sit on the map write stream, not on their reads, and the second animation of the spectrum is paid in full;
    // profiles/r05_4096_experiments.txt.  Of the per-launch fields it needed, rec_mode is still part of every launch: which launch is the frame's last
    // depends on the form; the mask of x-axis roles went with it, the mask of transforms is always 15 and only k_zpass_c1 still tests it: FrameArgs::zmask.)
    // Merged x pass (round 5): HEIGHT, NORMAL and DISP workgroups in ONE launch of k_xpass_b (xb_disp) instead of k_xpass_b + k_xpass_disp.
    // The DISP workgroups transform pair 0 at once and wait for the tile's HEIGHT workgroups only before their stores (raw heights handed over
    // write-through, ocean_kernels.h: store_wt / wait_counter): a small single tile is three short DEPENDENT latency chains
    // (profiles/r02_small_tile_experiments.txt item 0), and this runs the third one beside the second.  Where every workgroup of the launch
    // is resident at once, one per compute unit (the regime the hand-off recipe is measured for: MI355X_MICROARCH.md), a single tile, not
    // the Jacobian mode (its displacement pass also needs the NORMAL workgroups' product plane).  Same arithmetic per texel: same bits.
    // Where it pays (profiles/r05_small_tile_experiments.txt): a SERIAL frame only up to 128^2 (64^2: 12.8 -> 11.6 us; from 256^2 up the
    // hand-off's three dependent memory round trips cost more than the kernel boundary they replace: 512^2 16.6 -> 18.2 us); PIPELINED frames
    // of one tile up to 512^2, which are bound by the rate of launches, not by any kernel (512^2, depth 4: 13.2-14.9 -> 8.0 us per frame).
    bool merged_x = xmerge_pays<N>(alone) && tiles == 1 && a.mode != 3 && c->merged_x &&
                    xg <= c->tune.handoff_wg_per_cu * cus;
    // ONE launch for the whole frame (k_frame; round 5): pipelined frames of one tile up to 128^2 in the usual form (fp32 spectrum with 16-bit
    // dispersion, fp32 intermediates, both maps streamed, not the Jacobian mode) -- they are bound by the rate of launches.  Measured at depth 4,
    // us per frame, three launches / merged x pass / one launch: 64^2 11.5 / 7.6 / 3.9, 128^2 15.0 / 10.3 / 5.2 -- and 256^2 8.2-15.4 / 5.8 / 8.3,
    // 512^2 11.6-12.3 / 7.7 / 18.6: from 256^2 up the z pass's 8-byte write-through stores and the x-axis workgroups' reads past the L2 cost more
    // than the launch they save (profiles/r05_small_tile_experiments.txt), so those sizes keep the merged x pass.
    constexpr bool HAS_ONE = (N <= 128 || (DEV && N <= 512)) && G::T_ROWS == G::T_C;      // (developer builds: up to 512^2, for the A/B of that log)
    // (fp32 intermediates and never the Jacobian mode: the one-launch records of ocean_last_launch, below, rely on `describe` adding neither flag)
    // (like the merged x pass only where every workgroup of the grid has a slot at once -- one per compute unit, the regime the hand-off recipe is
    //  measured for: forward progress then never depends on the order in which workgroups are dispatched)
    bool one_launch = HAS_ONE && !alone && tiles == 1 && a.mode <= 2 && fast && p.nt_normal && p.nt_disp && !p.nt_inter && !p.half_inter && c->merged_x &&
                      ((unsigned)(N / 2 + 1) + xg) <= c->tune.handoff_wg_per_cu * cus;
    // the DISP workgroups of a merged launch poll the HEIGHT count; beside other chains' launches a poll every ~3 us instead of back to back
    // takes the pollers off the memory system (512^2 depth 4: 7.66-7.97 -> 7.35-7.55 us per frame, 256^2 7.8-9.7 -> 7.2-7.3); a serial frame
    // (<= 128^2) keeps the tight poll -- there the wait IS the frame's latency -- and so does a one-launch frame
    int poll_sleep = (merged_x && !one_launch && !alone) ? 1 : 0;
#ifdef OCEAN_DEVELOPER      // A/B builds only: the shipped library reads no environment.  Every override of the rules above, in their order
    {   static const char* const c1_env = getenv("OCEAN_ZC1");                  // 0 / 1
        if (c1_env && HASC1) c1 = atoi(c1_env) != 0;
        zw2 = HAS2 && !c1 && p.nt_inter;
        static const char* const zw_env = getenv("OCEAN_ZW");                   // 1 or 2
        if (zw_env && HAS2 && !c1) zw2 = atoi(zw_env) == 2;
        const char* const wt_env = getenv("OCEAN_Z_WT");          // 0: off (read per frame: A/B inside one process)
        z_wt = c1 && wt_frame && !(wt_env && atoi(wt_env) == 0);
        const char* const xm = getenv("OCEAN_XMERGE");            // 0 / 1: force (any size, any batch; still not the Jacobian mode)
        if (xm) merged_x = atoi(xm) != 0 && a.mode != 3;
        const char* const ol = getenv("OCEAN_ONE_LAUNCH");        // 0 / 1 (the form's own preconditions still hold)
        if (ol) one_launch = one_launch && atoi(ol) != 0;
        const char* const ps = getenv("OCEAN_POLL_SLEEP");
        poll_sleep = ps ? atoi(ps) : (merged_x && !one_launch && !alone) ? 1 : 0;
        static const char* const rz = getenv("OCEAN_RAMP_Z"); static const char* const rb = getenv("OCEAN_RAMP_B"); static const char* const rd = getenv("OCEAN_RAMP_D");
        static const char* const ra = getenv("OCEAN_RAMP_ANY");     // 1: every size and batch
        const bool on = ramp_z || ramp_b || ramp_d || (ra && atoi(ra) == 1);
        if (rz && on) ramp_z = atoi(rz);
        if (rb && on) ramp_b = atoi(rb);
        if (rd && on) ramp_d = atoi(rd); }
#endif
    fl.handoff = merged_x || one_launch;      // (what recover_fault re-runs without a hand-off, should one of this frame's in-launch waits give up)
    fl.launch_count = 0;
    auto next_marks = [&](int kernel) -> hipEvent_t* {      // the event pair of the frame's next launch; remembers which kernel it times
        const int l = fl.launch_count++;
        fl.launch_kernel[l] = kernel;
        return fl.marks ? fl.marks + 2 * l : nullptr;
    };
    // what ocean_last_launch reports of launch idx: the caller passes what differs between the launches, the flags of the frame's form are added here
    auto describe = [&](int idx, unsigned grid_x, unsigned block, unsigned per_workgroup, size_t lds, uint32_t flags) {
        ocean_launch_info& li = c->last_launch[idx];
        li.tile_size = N; li.grid_x = grid_x; li.grid_y = tiles; li.block = block; li.mode = (uint32_t)a.mode;
        li.per_workgroup = per_workgroup;
        li.lds_bytes = (uint32_t)lds;
        li.flags = flags | (p.half_inter ? OCEAN_LAUNCH_HALF_INTER : 0u) | (a.mode == 3 ? OCEAN_LAUNCH_JACOBIAN : 0u);
    };
    const int rec_last = a.rec_mode;                         // what the frame's LAST launch does with the completion records (ocean_api.hip)
    auto launch_z = [&]() -> hipError_t {
        const unsigned gx = zw2 ? N / 4 + 1 : N / 2 + 1;
        FrameArgs za = a;
        za.rec_mode = 0;
        // one 2048^2 tile: the single-transform form's 1025 workgroups are one resident round -- staggered start (start_ramp_wait)
        za.start_ramp = c1 ? ramp_z : 0;
        const unsigned threads = c1 ? (unsigned)zpass_c1_threads<N>() : (unsigned)G::T_ROWS;
        const size_t lds = c1 ? zpass_c1_lds_bytes<N>() : (zw2 ? lds_rows2 : lds_rows);
        const dim3 grid(gx, tiles), block(threads);
        describe(0, gx, threads, zw2 ? 2u : 1u, lds,
                 (p.nt_inter ? OCEAN_LAUNCH_NT_INTER : 0u) | (a.h0h ? OCEAN_LAUNCH_FP16_SPECTRUM : 0u) |
                 (a.omega_q ? 0u : OCEAN_LAUNCH_FP32_DISPERSION) | (c1 ? OCEAN_LAUNCH_SINGLE_TRANSFORM : 0u) |
                 (za.start_ramp ? OCEAN_LAUNCH_STAGGERED_START : 0u) | (z_wt ? OCEAN_LAUNCH_WT_INTER : 0u));
        hipEvent_t* mz = next_marks(0);
#ifdef OCEAN_CLOCKPROBE
        {   // diagnostic: this translation unit's copy of the probe pointer, set when the context's buffer changes (not per frame)
            static unsigned long long* armed = nullptr;
            if (armed != c->stamps) { armed = c->stamps; (void)hipMemcpyToSymbol(HIP_SYMBOL(ocean::g_clockprobe), &armed, sizeof(armed)); }
        }
#endif
        bool launched = false;
        if constexpr (HAS_WT) {
            if (z_wt) {
                if (fast) launch(k_zpass_c1<N, zpass_c1_threads<N>(), typename C1Plan<N>::type, false, false, true, true>, grid, block, lds, st, mz, za);
                else launch(k_zpass_c1<N, zpass_c1_threads<N>(), typename C1Plan<N>::type, false, false, false, true>, grid, block, lds, st, mz, za);
                launched = true;
            }
        }
#define OCEAN_ZPASS3(znt, z16, fast) \
        do { if (launched) break; if constexpr (HASC1) { if (c1) { launch(k_zpass_c1<N, zpass_c1_threads<N>(), typename C1Plan<N>::type, znt, z16, fast>, grid, block, lds, st, mz, za); launched = true; break; } } \
             if constexpr (HAS2 && (znt || HAS2_PLAIN)) { if (zw2) { launch(k_zpass<N, G::T_ROWS, typename G::PR, znt, z16, 2, fast>, grid, block, lds, st, mz, za); launched = true; break; } } \
             if constexpr (HAS1) { if (!c1 && !zw2) { launch(k_zpass<N, G::T_ROWS, typename G::PR, znt, z16, 1, fast>, grid, block, lds, st, mz, za); launched = true; } } } while (0)
#define OCEAN_ZPASS2(znt, z16) \
        do { if (fast) OCEAN_ZPASS3(znt, z16, true); else OCEAN_ZPASS3(znt, z16, false); } while (0)
#define OCEAN_ZPASS(znt) \
        do { if (p.half_inter) OCEAN_ZPASS2(znt, true); else OCEAN_ZPASS2(znt, false); } while (0)
        if (p.nt_inter) OCEAN_ZPASS(true); else OCEAN_ZPASS(false);
#undef OCEAN_ZPASS
#undef OCEAN_ZPASS2
#undef OCEAN_ZPASS3
        if (!launched) return hipErrorInvalidConfiguration;     // (a form this build does not carry: the rules above never ask for one)
        return hipSuccess;
    };
    const bool jac = a.mode == 3;       // OCEAN_MODE_JACOBIAN: the height role works on pair 3, C rows per workgroup
    const unsigned hb = jac ? nb : hb_b;
    const dim3 blk(G::T_C);
#define OCEAN_XPASS2(kern, grid, lds, ev, nts, z16, args)                                                          \
        do { if (jac) launch(kern<N, C, G::T_C, typename G::PC, nts, z16, true>, grid, blk, lds, st, ev, args);       \
             else launch(kern<N, C, G::T_C, typename G::PC, nts, z16, false>, grid, blk, lds, st, ev, args); } while (0)
#define OCEAN_XPASS(kern, grid, lds, ev, nts, args)                                                                 \
        do { if (p.half_inter) OCEAN_XPASS2(kern, grid, lds, ev, nts, true, args);                                  \
             else OCEAN_XPASS2(kern, grid, lds, ev, nts, false, args); } while (0)
    auto launch_xb = [&](bool merged) {      // HEIGHT + NORMAL workgroups; merged: the DISP workgroups as well -- then the frame's last launch
        const dim3 gb(hb + nb + (merged ? nb : 0u), tiles);
        const uint32_t flags_b = (ramp_b ? OCEAN_LAUNCH_STAGGERED_START : 0u) | (merged ? OCEAN_LAUNCH_MERGED_X : 0u);
        describe(1, gb.x, G::T_C, C, lds_b, flags_b | (p.nt_normal ? OCEAN_LAUNCH_NT_MAPS : 0u));
        // no k_xpass_disp this frame: its record describes the launch that did its work
        if (merged) describe(2, gb.x, G::T_C, C, lds_b, flags_b | (p.nt_disp ? OCEAN_LAUNCH_NT_MAPS : 0u));
        hipEvent_t* mb = next_marks(1);
        FrameArgs ba = a;
        ba.xb_disp = merged ? 1 : 0; ba.rec_mode = merged ? rec_last : 0;
        ba.poll_sleep = poll_sleep;
        ba.start_ramp = ramp_b;             // over its normal-map workgroups (the height workgroups start at once)
        if (p.nt_normal) OCEAN_XPASS(k_xpass_b, gb, lds_b, mb, true, ba);
        else OCEAN_XPASS(k_xpass_b, gb, lds_b, mb, false, ba);
    };
    auto launch_xd = [&]() {
        const dim3 gd(nb, tiles);
        describe(2, gd.x, G::T_C, C, lds_m, (p.nt_disp ? OCEAN_LAUNCH_NT_MAPS : 0u) | (ramp_d ? OCEAN_LAUNCH_STAGGERED_START : 0u));
        hipEvent_t* md = next_marks(2);
        FrameArgs da = a;
        da.rec_mode = rec_last;
        da.start_ramp = ramp_d;             // its 257 workgroups are one per CU: the same read-then-write burst
        if (p.nt_disp) OCEAN_XPASS(k_xpass_disp, gd, lds_m, md, true, da);
        else OCEAN_XPASS(k_xpass_disp, gd, lds_m, md, false, da);
    };
    if constexpr (HAS_ONE) {
        if (one_launch) {
            constexpr size_t lds_one = lds_rows > lds_b ? lds_rows : lds_b;
            auto kern = k_frame<N, C, G::T_C, typename G::PR, typename G::PC, true, false, true>;
            if (c->attr_one_n != (uint32_t)N) {
                if ((e = allow_lds(kern, lds_one)) != hipSuccess) return e;
                c->attr_one_n = (uint32_t)N;
            }
            FrameArgs fa = a;
            fa.xb_disp = 1; fa.rec_mode = rec_last; fa.start_ramp = 0;
            fa.zdone_target = (++c->zgen[fl.set]) * (unsigned)(N / 2 + 1);
            fa.poll_sleep = poll_sleep;
            const dim3 grid((N / 2 + 1) + xg, tiles), block(G::T_C);
            // (describe adds nothing: the one_launch rule above excludes half2 intermediates and the Jacobian mode)
            for (int k = 0; k < 3; ++k)
                describe(k, grid.x, G::T_C, k == 0 ? 1u : (unsigned)C, lds_one, OCEAN_LAUNCH_ONE_LAUNCH | (k == 0 ? 0u : (OCEAN_LAUNCH_NT_MAPS | OCEAN_LAUNCH_MERGED_X)));
            launch(kern, grid, block, lds_one, st, next_marks(0), fa);
            if (fl.after_z && (e = hipEventRecord(fl.after_z, st)) != hipSuccess) return e;
            return hipGetLastError();
        }
    }
    if ((e = launch_z()) != hipSuccess) return e;
    if (fl.after_z && (e = hipEventRecord(fl.after_z, st)) != hipSuccess) return e;   // the first frames after a drain: the next chain's z pass starts behind this one (ocean_api.hip)
    if (merged_x) {
        launch_xb(true);
    } else {
        launch_xb(false);
        // the normal map is final behind this launch: ocean_compute_waves_read starts its device-to-host copy here, beside the displacement pass
        if (fl.after_b) { if ((e = hipEventRecord(fl.after_b, st)) != hipSuccess) return e; fl.after_b_recorded = true; }
        launch_xd();
    }
#undef OCEAN_XPASS2
#undef OCEAN_XPASS
    return hipGetLastError();
}

