// Host selftest of fps_plan (epnet_amd/csrc/fps_plan.h), the decision behind the five sampling entry points.
//   rows                  one line per call of the boundary table: what test_fps_plan.py pins (recorded from the dispatch code
//                         this plan replaced)
//   sweep LO HI           every n in [LO, HI] crossed with the sample counts, the pointer patterns the entry points allow and every
//                         legal knob value: asserts the invariants the kernels rely on, prints the (family, waves, ppt) ever chosen
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "fps_plan.h"

using namespace epnet;

static const char *const kFamily[] = {"none", "wave", "pruned", "indexed", "bigscene", "stream"};
static const char *const kEntry[] = {"fps", "fps_indexed", "centres", "chain", "chain_index"};

// the optional pointers of an entry point, as bits of a pattern: every combination is a legal call
enum { kIndex = 1, kTemp = 2, kNewXyz = 4, kPrefixIn = 8, kPrefixOut = 16, kNoXyz = 32 };
static const int kOptional[] = {kTemp, kIndex | kTemp | kNoXyz, kIndex | kTemp, kIndex | kTemp | kNewXyz | kPrefixIn | kPrefixOut,
                                kIndex | kTemp | kPrefixIn | kPrefixOut};
// what else a call may get wrong: a workspace one byte short, a misaligned next_index, a required pointer left out
enum Flaw { kSound, kShortIndex, kShortNext, kMisaligned, kNoIdx, kNoNewXyz, kFlaws };

static FpsCall make_call(int entry, int b, int n, int m, int pattern, int cap, int flaw = kSound) {
    FpsCall c = {};
    c.entry = (FpsEntry)entry;
    c.b = b, c.n = n, c.m = m;
    c.xyz = !(pattern & kNoXyz);
    c.idx = flaw != kNoIdx;
    c.index = pattern & kIndex, c.temp = pattern & kTemp;
    c.new_xyz = entry == kFpsEntryCentres || entry == kFpsEntryChainIndex || (pattern & kNewXyz);
    if (flaw == kNoNewXyz) c.new_xyz = false;
    c.prefix_in = pattern & kPrefixIn, c.prefix_out = pattern & kPrefixOut;
    c.next_index = entry == kFpsEntryChainIndex;
    c.next_index_aligned = flaw != kMisaligned;
    c.index_bytes = c.index ? scene_index_bytes(b, n) - (flaw == kShortIndex) : 0;
    c.next_index_bytes = c.next_index ? scene_index_bytes(b, m) - (flaw == kShortNext) : 0;
    c.prefix_cap = entry >= kFpsEntryChain ? cap : 0x7fffffff;
    return c;
}

// f(call, pattern) for every pattern of every entry point
template <class F>
static void for_each_pattern(int b, int n, int m, int cap, F &&f) {
    for (int entry = 0; entry < 5; ++entry)
        for (int pattern = 0; pattern < 64; ++pattern)
            if ((pattern & ~kOptional[entry]) == 0) f(make_call(entry, b, n, m, pattern, cap), pattern);
}

static int g_failures = 0;
#define CHECK(cond, c, p)                                                                                                         \
    do {                                                                                                                          \
        if (!(cond) && ++g_failures <= 20)                                                                                        \
            printf("FAILED %s: %s b=%d n=%d m=%d -> %s<%d,%d>\n", #cond, kEntry[(c).entry], (c).b, (c).n, (c).m, kFamily[(p).family], \
                   (p).waves, (p).ppt);                                                                                           \
    } while (0)

// what the kernels and the sampling chain rely on, and what fps_run's ladders instantiate
static void check_invariants(const FpsCall &c, const FpsPlan &p) {
    if (p.rc != EPNET_OK) {
        CHECK(p.family == kFpsNone && p.follow == kFpsNothing && p.prefix_init < 0, c, p);
        return;
    }
    if (p.family == kFpsNone) {
        CHECK((c.b == 0 || c.m == 0) && p.follow == kFpsNothing && p.prefix_init < 0, c, p);
        return;
    }
    // the index epilogue: 8 centres per thread of the 512-thread kernel, and every scene must reach the kernel's tail
    if (p.builds_next)
        CHECK(p.family == kFpsIndexed && c.m >= 1024 && c.m <= 4096 && !p.prefix_in && scene_index_np(c.n) == 16384 && p.waves == 8 &&
                  c.next_index && c.new_xyz,
              c, p);
    // prefix_out starts at m only under a kernel that lowers it at a tie: elsewhere the chain would take the identity wrongly
    if (p.prefix_init == c.m || p.prologue_init == c.m) CHECK(fps_reports_ties(p.family), c, p);
    CHECK(p.prefix_init < 0 || p.prologue_init < 0, c, p);
    CHECK((p.prefix_init >= 0 || p.prologue_init >= 0) == (p.prefix_in || c.prefix_out), c, p);
    if (p.prologue_init >= 0) CHECK(p.family == kFpsWave || p.family == kFpsIndexed, c, p);
    if (p.prefix_in) CHECK(c.m <= c.n, c, p);
    // the running distances in memory
    if (!c.temp) CHECK(p.family != kFpsStream && p.family != kFpsBigscene, c, p);
    if (p.family == kFpsIndexed || p.family == kFpsBigscene) CHECK(c.index && c.index_bytes >= scene_index_bytes(c.b, c.n), c, p);
    // the centres are written exactly once, by whoever the plan names
    if (c.new_xyz) CHECK((int)p.writes_centres + (int)p.builds_next + (p.follow != kFpsNothing) >= 1, c, p);
    if (c.next_index) CHECK(p.builds_next != (p.follow == kFpsIndexBuild), c, p);
    if (p.follow == kFpsGather) CHECK(c.new_xyz && !p.writes_centres && c.b <= 65535, c, p);
    // capacity of the instantiation
    switch (p.family) {
        case kFpsWave: {
            const int bs = 1 << p.lg_bs, J = (c.n + bs - 1) / bs;
            CHECK(64 * p.waves <= bs && bs / (64 * p.waves) * J <= p.ppt && p.ppt <= 16 && p.lds == 0, c, p);
            break;
        }
        case kFpsPruned:
            CHECK((p.waves == 4 || p.waves == 8) && (p.ppt == 8 || p.ppt == 16 || p.ppt == 32) && 64 * p.waves * p.ppt >= c.n &&
                      p.lds <= 160 * 1024 && c.n <= 16384,
                  c, p);
            break;
        case kFpsIndexed: CHECK(64 * p.waves * p.ppt == scene_index_np(c.n) && c.n > 1024 && c.n <= 16384 && c.m > 1, c, p); break;
        case kFpsBigscene: CHECK(p.waves == 16 && c.n > 16384 && c.n <= 65536 && c.xyz, c, p); break;
        case kFpsStream: CHECK(p.waves >= 1 && p.waves <= 16 && (64 * p.waves) % (1 << p.lg_bs) == 0, c, p); break;
        default: break;
    }
}

static void print_row(const char *knob_tag, const FpsCall &c, int pattern, int flaw, const FpsPlan &p) {
    printf("%s %s b=%d n=%d m=%d p=%d f=%d cap=%d :", knob_tag, kEntry[c.entry], c.b, c.n, c.m, pattern, flaw, c.prefix_cap);
    if (p.rc != EPNET_OK || p.family == kFpsNone) {
        printf(" rc=%d\n", p.rc);
        return;
    }
    const bool takes_cap = p.family == kFpsPruned || p.family == kFpsIndexed;
    printf(" rc=0 %s<%d,%d> lg=%d lds=%zu prefix=%d prologue=%d cap=%d in=%d centres=%d next=%d follow=%d\n", kFamily[p.family], p.waves,
           p.ppt, p.lg_bs, p.lds, p.prefix_init, p.prologue_init, takes_cap ? p.prefix_cap : 0, (int)p.prefix_in, (int)p.writes_centres,
           (int)p.builds_next, (int)p.follow);
}

static const FpsKnobs kDefault = {1, 1024, -1, -1};

static int rows() {
    static const int ns[] = {1, 63, 64, 65, 127, 128, 512, 513, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 65536, 65537};
    static const struct { const char *tag; FpsKnobs knobs; } configs[] = {
        {"default", kDefault}, {"prune=0", {0, 1024, -1, -1}}, {"prune_min=4096", {1, 4096, -1, -1}},
        {"pwaves=8", {1, 1024, 8, -1}}, {"waves=4", {1, 1024, -1, 4}}};
    for (const auto &cfg : configs)
        for (int n : ns) {
            const int ms[] = {0, 1, 2, 1023, 1024, 4096, 4097, n, n + 1};
            for (int m : ms)
                for (int b : {2, 513}) {
                    for_each_pattern(b, n, m, (n & 1) ? 0 : 64, [&](const FpsCall &c, int pattern) {
                        const FpsPlan p = fps_plan(c, cfg.knobs);
                        check_invariants(c, p);
                        print_row(cfg.tag, c, pattern, kSound, p);
                    });
                    if (b != 2 || &cfg != configs) continue;
                    for (int entry = 0; entry < 5; ++entry)   // the flawed calls, with every optional pointer given
                        for (int flaw = 1; flaw < kFlaws; ++flaw) {
                            const int pattern = kOptional[entry] & ~kNoXyz;
                            const FpsCall c = make_call(entry, b, n, m, pattern, 64, flaw);
                            print_row(cfg.tag, c, pattern, flaw, fps_plan(c, cfg.knobs));
                        }
                }
        }
    for (int b : {0, 65535, 65536})   // the limits on the number of scenes
        for (int n : {1000, 5000, 20000})
            for_each_pattern(b, n, 1024, 64, [&](const FpsCall &c, int pattern) { print_row("default", c, pattern, kSound, fps_plan(c, kDefault)); });
    return g_failures != 0;
}

static int sweep(int lo, int hi) {
    static bool chosen[6][17][33];
    static const int prune_mins[] = {0, 1024, 5000, 0x7fffffff};
    long long plans = 0;
    for (int n = lo; n <= hi; ++n) {
        const int ms[] = {0, 1, 2, 64, 1024, 4096, n, n + 1};
        for (int m : ms)
            for (int prune = 0; prune <= 1; ++prune)
                for (int prune_min : prune_mins)
                    for (int pwaves : {-1, 4, 8})
                        for (int waves : {-1, 1, 2, 4, 8, 16}) {
                            if (!prune && (prune_min != 1024 || pwaves != -1)) continue;   // (neither is read with the pruning off)
                            const FpsKnobs knobs = {prune, prune_min, pwaves, waves};
                            const bool dflt = prune && prune_min == 1024 && pwaves == -1 && waves == -1;
                            for (int b : {2, 513, 65536}) {
                                if (b != 2 && !dflt) continue;   // (b enters through the knob-free limits and the 512-scene rule)
                                for_each_pattern(b, n, m, (n & 1) ? 0 : 64, [&](const FpsCall &c, int) {
                                    const FpsPlan p = fps_plan(c, knobs);
                                    check_invariants(c, p);
                                    chosen[p.family][p.waves][p.ppt] = true;
                                    ++plans;
                                });
                            }
                        }
    }
    printf("plans %lld\n", plans);
    for (int f = 1; f < 6; ++f)
        for (int w = 0; w <= 16; ++w)
            for (int t = 0; t <= 32; ++t)
                if (chosen[f][w][t]) printf("chosen %s<%d,%d>\n", kFamily[f], w, t);
    return g_failures != 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "rows")) return rows();
    if (argc == 4 && !strcmp(argv[1], "sweep")) return sweep(atoi(argv[2]), atoi(argv[3]));
    fprintf(stderr, "usage: %s rows | sweep LO HI\n", argv[0]);
    return 2;
}
