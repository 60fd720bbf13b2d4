// fps_plan.h -- which sampling kernel a call gets, and what runs in front of and behind it: pure integer logic on the shape, the
// NULL pattern of the pointers and the four tuning knobs. Free of HIP, so that a host test walks it exhaustively
// (tests/fps_plan_selftest.cpp); fps_run in fps.hip carries a plan out and decides nothing itself.
#pragma once
#include <math.h>
#include <stddef.h>

#include "epnet_ops.h"
#include "scene_index_layout.h"

namespace epnet {

// the entry point (which pointers it takes, and requires): epnet_furthest_point_sampling, ~_indexed, epnet_sample_centres, ~_chain, ~_chain_index
enum FpsEntry { kFpsEntryPlain, kFpsEntryIndexed, kFpsEntryCentres, kFpsEntryChain, kFpsEntryChainIndex };
enum FpsFamily { kFpsNone, kFpsWave, kFpsPruned, kFpsIndexed, kFpsBigscene, kFpsStream };
enum FpsFollow { kFpsNothing, kFpsGather, kFpsIndexBuild };   // behind the sampling kernel: gather_centres / the gathered index build

struct FpsCall {
    FpsEntry entry;
    int b, n, m;
    size_t index_bytes, next_index_bytes;
    bool xyz, index, temp, idx, new_xyz, prefix_in, prefix_out, next_index;   // non-NULL?
    bool next_index_aligned;                                                   // to 16 bytes
    int prefix_cap;
};
struct FpsKnobs { int prune, prune_min, pwaves, waves; };   // tuning(kFpsPrune | kFpsPruneMin | kFpsPwaves | kFpsWaves)

struct FpsPlan {
    int rc;              // nothing is launched unless EPNET_OK (nor for an empty problem: family kFpsNone)
    FpsFamily family;
    int waves, ppt;      // the instantiation (stream, bigscene: waves = workgroup size / 64, ppt = 0)
    int lg_bs;           // log2 of the reference's block size, which defines the tie-break (wave, stream)
    size_t lds;          // dynamic LDS bytes
    int prefix_init;     // >= 0: fps_prefix_kernel runs in front, with this initial value of prefix_out
    int prologue_init;   // >= 0: the kernel does that itself (fps_prologue)
    int prefix_cap;
    bool prefix_in;      // the known prefixes are used (dropped for m > n: the sequence repeats points, nothing is known)
    bool writes_centres; // the sampling kernel writes new_xyz itself
    bool builds_next;    // ... and next_index, in its epilogue
    FpsFollow follow;
};

// does the family report its tie-free rounds by lowering prefix_out? (the others leave it at its initial value)
inline bool fps_reports_ties(FpsFamily f) { return f == kFpsPruned || f == kFpsIndexed; }

// opt_n_threads, pointnet2_lib/pointnet2/src/cuda_utils.h:10-14 -- same double-precision libm
// formula as the reference's host code, so the block size that defines the tie-break is the same.
inline int ref_block_lg(int work_size) {
    int pow_2 = (int)(log(static_cast<double>(work_size)) / log(2.0));
    if (pow_2 > 10) pow_2 = 10;
    if (pow_2 < 0) pow_2 = 0;
    return pow_2;
}

inline FpsPlan fps_no_launch(int rc) { return FpsPlan{rc, kFpsNone, 0, 0, 0, 0, -1, -1, 0x7fffffff, false, false, false, kFpsNothing}; }

inline FpsPlan fps_plan(const FpsCall &c, const FpsKnobs &knobs) {
    const int b = c.b, n = c.n, m = c.m;
    if (!(b >= 0 && n >= 1 && m >= 0)) return fps_no_launch(EPNET_EINVAL);
    if (b == 0 || m == 0) return fps_no_launch(EPNET_OK);  // the reference kernel returns at once for m <= 0
    // over a scene index: 1024 < n <= 65536 (for n <= 1024 the reference block size, hence the tie-break rank, depends on n: the
    // wave kernel handles it), and beyond 16384 points only with the running distances in memory
    const size_t need = scene_index_bytes(b, n);
    const bool over_index = need != 0 && c.index && n > 1024 && m > 1 && (n <= 16384 || c.temp);
    // (the indexed entry point reads xyz only where the kernel does: required below for the bigscene family alone)
    if (!c.idx || !(c.xyz || (c.entry == kFpsEntryIndexed && over_index))) return fps_no_launch(EPNET_EINVAL);
    if (c.entry == kFpsEntryCentres && !c.new_xyz) return fps_no_launch(EPNET_EINVAL);
    if (c.entry == kFpsEntryChainIndex && !(c.new_xyz && c.next_index)) return fps_no_launch(EPNET_EINVAL);
    if (c.next_index) {   // 1024 <= m <= 16384, new_xyz required
        const size_t need2 = scene_index_bytes(b, m);
        if (need2 == 0 || m > 16384 || !c.new_xyz || b > 65535) return fps_no_launch(EPNET_EINVAL);
        if (c.next_index_bytes < need2) return fps_no_launch(EPNET_ENOMEM);
        if (!c.next_index_aligned) return fps_no_launch(EPNET_EINVAL);
    }
    FpsPlan p = fps_no_launch(EPNET_OK);
    p.prefix_in = c.prefix_in && m <= n;
    const bool prefixes = p.prefix_in || c.prefix_out;
    if (prefixes && b > 65535) return fps_no_launch(EPNET_EINVAL);
    p.prefix_cap = prefixes && c.prefix_cap < 1 ? 0x7fffffff : c.prefix_cap;

    const int lg = ref_block_lg(n), bs_ref = 1 << lg, J = (int)(((long long)n + bs_ref - 1) / bs_ref);
    if (over_index) {
        if (c.index_bytes < need) return fps_no_launch(EPNET_ENOMEM);
        const int np = scene_index_np(n);
        if (n > 16384) {  // beyond the register file: bucket summaries in registers, points re-read from the index
            if (!c.xyz) return fps_no_launch(EPNET_EINVAL);
            p.family = kFpsBigscene;
            p.waves = 16;
        } else {
            p.family = kFpsIndexed;
            p.waves = np == 16384 ? 8 : 4;
            p.ppt = np / (64 * p.waves);
            // The 512-thread kernel builds the scene index of its m centres in its epilogue, 8 centres per thread: 1024 <= m <=
            // 4096, and every scene must run the kernel's tail (no known prefixes: a scene taking the identity leaves early).
            // (The centres alone come from the small gather: written by the sampling kernel itself they cost wave 0 an LDS write
            // per round and 12 KB more LDS, 1.7 % on one scene and 5 % in the software-pipelined stack -- more than the launch)
            p.builds_next = c.next_index && !p.prefix_in && np == 16384 && m >= 1024 && m <= 4096;
        }
    } else if ((long long)n > (1ll << 20) * 1024) {
        return fps_no_launch(EPNET_ELIMIT);  // rank field: 20 bits of k div bs
    } else if (knobs.prune != 0 && n > 1024 && n > knobs.prune_min && n <= 16384 && m > 1) {
        // the exact spatially-pruned kernel, self-sorting (EPNET_FPS_PRUNE=0 forces the brute-force path, EPNET_FPS_PRUNE_MIN
        // raises the lower end). 64-point slots: 4 waves x {8,16,32} slots, 8 waves above 8192 points (EPNET_FPS_PWAVES overrides)
        p.family = kFpsPruned;
        p.waves = n > 8192 ? 8 : 4;
        const int w = knobs.pwaves;
        if (w > 0 && (n + 64 * w - 1) / (64 * w) <= 32) p.waves = w;
        const int ppt_need = (n + 64 * p.waves - 1) / (64 * p.waves);
        p.ppt = ppt_need <= 8 ? 8 : ppt_need <= 16 ? 16 : 32;
        p.lds = (size_t)(kCells + kCells / (kCells / (64 * p.waves)) + 64) * sizeof(int) + (size_t)64 * p.waves * p.ppt * 2;
    } else if (bs_ref >= 64 && J <= 16) {
        p.family = kFpsWave;
        p.lg_bs = lg;
        // fewest waves whose threads can hold the scene in <= 16 slots each (fewer waves = cheaper
        // cross-wave exchange and more scenes per CU); EPNET_FPS_WAVES overrides for tuning
        p.waves = bs_ref / 64;
        for (int w = 1; w <= bs_ref / 64; w *= 2)
            if ((bs_ref / (64 * w)) * J <= 16) {
                p.waves = w;
                break;
            }
        // few scenes of 512 < n <= 1024 points: the chip is idle anyway and a round is shorter with 2 slots per
        // thread on 8 waves (0.48 us) than with 16 slots on one wave (0.66 us); many small scenes pack best at 1 wave
        if (n > 512 && b <= 512 && bs_ref / 64 >= 8 && p.waves < 8) p.waves = 8;
        const int w = knobs.waves;  // (a power of two, or -1)
        if (w >= 1 && w <= bs_ref / 64 && (bs_ref / (64 * w)) * J <= 16) p.waves = w;
        const int slots = (bs_ref / (64 * p.waves)) * J;
        p.ppt = slots <= 1 ? 1 : slots <= 2 ? 2 : slots <= 4 ? 4 : slots <= 8 ? 8 : 16;
        p.writes_centres = c.new_xyz;
    } else {  // generic path: needs the running distances in memory (temp may only be NULL on the register-resident paths)
        if (!c.temp) return fps_no_launch(EPNET_EINVAL);
        p.family = kFpsStream;
        p.lg_bs = lg;
        p.waves = bs_ref < 64 ? 1 : bs_ref / 64;
    }
    // the known prefixes / the tie-free counts want their initial treatment: prefix_out starts at m where the kernel reports ties
    // by lowering it, at 0 where it cannot tell -- folded into the kernels that have the prologue, a launch in front of the others
    if (prefixes) {
        const int init = fps_reports_ties(p.family) ? m : 0;
        if (p.family == kFpsWave || p.family == kFpsIndexed) p.prologue_init = init;
        else p.prefix_init = init;
    }
    // what the epilogue does not build: gather + index build in one dispatch (a sampling kernel that wrote the centres itself
    // wrote the same rows), or the gather alone
    if (c.next_index) p.follow = p.builds_next ? kFpsNothing : kFpsIndexBuild;
    else if (c.new_xyz && !p.writes_centres) p.follow = kFpsGather;
    if (p.follow == kFpsGather && b > 65535) return fps_no_launch(EPNET_EINVAL);
    return p;
}

}  // namespace epnet
