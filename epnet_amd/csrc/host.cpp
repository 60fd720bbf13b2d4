// host.cpp -- the non-kernel part of libepnet_hip.so: ABI bookkeeping, error strings and the two
// roipool3d ops that are HOST-memory ops in the reference itself (roipool3d.cpp:97-195; they run
// inside DataLoader worker processes, lib/datasets/kitti_rcnn_dataset.py:672,767,811,1029,1157).
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "common.h"
#include "cr_trig.h"

namespace epnet {

static thread_local std::string g_last_hip_error;

int record_hip_error(hipError_t e, const char *where) {
    g_last_hip_error = std::string(where) + ": " + hipGetErrorString(e);
    return EPNET_ELAUNCH;
}

// ---- kernel-selection overrides (epnet_set_tuning; the knobs are listed in epnet_ops.h)
static const struct {
    const char *name;
    int lo, hi, dflt;  // accepted values besides -1; what tuning() reports without an override (-1: the launcher decides)
} kKnobs[kKnobCount] = {  // in Knob order
    {"EPNET_FPS_PRUNE", 0, 1, 1},     {"EPNET_FPS_PRUNE_MIN", 0, INT_MAX, 1024}, {"EPNET_FPS_PWAVES", 4, 8, -1},
    {"EPNET_FPS_WAVES", 1, 16, -1},   {"EPNET_BQ_PAIR", 0, 1, -1},               {"EPNET_BQ_STREAM", 0, 1, -1},
    {"EPNET_BQ_ORDERED", 0, 1, -1},   {"EPNET_NN_TILE_MIN_BUCKETS", 0, INT_MAX, 4096},
};
static std::atomic<int> g_knob[kKnobCount];  // -1: no override

static bool knob_accepts(int k, long v) {  // (wave counts: powers of two)
    const bool pow2 = k == kFpsPwaves || k == kFpsWaves;
    return v == -1 || (v >= kKnobs[k].lo && v <= kKnobs[k].hi && (!pow2 || (v & (v - 1)) == 0));
}

static int find_knob(const char *name) {
    for (int k = 0; name && k < kKnobCount; ++k)
        if (strcmp(name, kKnobs[k].name) == 0) return k;
    return -1;
}

// the only place the library reads its environment, once (an A/B run such as `EPNET_BQ_PAIR=1 python bench.py` needs no code
// change); a malformed or out-of-range value is ignored
static bool seed_from_env() {
    for (int k = 0; k < kKnobCount; ++k) {
        const char *e = getenv(kKnobs[k].name);
        char *end = nullptr;
        const long v = e ? strtol(e, &end, 10) : -1;
        g_knob[k].store(e && end != e && *end == '\0' && knob_accepts(k, v) ? (int)v : -1, std::memory_order_relaxed);
    }
    return true;
}

static std::atomic<int> &knob(int k) {
    static const bool seeded = seed_from_env();  // on first use; thread-safe (C++11)
    (void)seeded;
    return g_knob[k];
}

int tuning(Knob k) {
    const int v = knob(k).load(std::memory_order_relaxed);
    return v >= 0 ? v : kKnobs[k].dflt;
}

// pt_in_box3d_cpu, lib/utils/roipool3d/src/roipool3d.cpp:82-95. The box-only terms are hoisted
// out of the point loop by the callers below (same values, computed once per box).
struct BoxTerms {
    float cx, cy, cz, hh, hw, hl, cosa, sina;
};

static inline BoxTerms box_terms(const float *b) {
    BoxTerms t;
    t.cx = b[0];
    t.cz = b[2];
    t.cy = (float)((double)b[1] - (double)b[3] / 2.0);
    t.hh = b[3] * 0.5f;
    t.hw = b[4] * 0.5f;
    t.hl = b[5] * 0.5f;
    cr_cossinf(b[6], t.cosa, t.sina);
    return t;
}

static inline int pt_in_box(const BoxTerms &t, float x, float y, float z) {
    const float max_dis = 10.0f;
    if ((fabsf(x - t.cx) > max_dis) || (fabsf(y - t.cy) > t.hh) || (fabsf(z - t.cz) > max_dis)) return 0;
    const float x_rot = (x - t.cx) * t.cosa + (z - t.cz) * (-t.sina);
    const float z_rot = (x - t.cx) * t.sina + (z - t.cz) * t.cosa;
    return (x_rot >= -t.hl) & (x_rot <= t.hl) & (z_rot >= -t.hw) & (z_rot <= t.hw);
}

}  // namespace epnet

using namespace epnet;

extern "C" int epnet_abi_version(void) { return EPNET_ABI_VERSION; }

extern "C" const char *epnet_strerror(int code) {
    switch (code) {
        case EPNET_OK: return "ok";
        case EPNET_EINVAL: return "invalid argument (negative size, NULL pointer, unknown tuning name or value)";
        case EPNET_ELAUNCH: return "HIP kernel launch failed";
        case EPNET_ENOMEM: return "workspace too small";
        case EPNET_ELIMIT: return "problem size outside the supported range";
        default: return "unknown epnet error code";
    }
}

extern "C" const char *epnet_last_hip_error(void) { return g_last_hip_error.c_str(); }

extern "C" int epnet_set_tuning(const char *name, int value) {
    const int k = find_knob(name);
    EPNET_REQUIRE(k >= 0 && knob_accepts(k, value));
    knob(k).store(value, std::memory_order_relaxed);
    return EPNET_OK;
}

extern "C" int epnet_get_tuning(const char *name, int *value) {
    const int k = find_knob(name);
    EPNET_REQUIRE(k >= 0 && value);
    *value = knob(k).load(std::memory_order_relaxed);
    return EPNET_OK;
}

extern "C" int epnet_pts_in_boxes3d_host(int64_t *pts_flag, const float *pts, const float *boxes3d, int64_t boxes_num,
                                         int64_t pts_num) {
    EPNET_REQUIRE(boxes_num >= 0 && pts_num >= 0);
    if (boxes_num == 0 || pts_num == 0) return EPNET_OK;
    EPNET_REQUIRE(pts_flag && pts && boxes3d);
    for (int64_t i = 0; i < boxes_num; ++i) {
        const BoxTerms t = box_terms(boxes3d + i * 7);
        int64_t *row = pts_flag + i * pts_num;
        for (int64_t j = 0; j < pts_num; ++j) row[j] = pt_in_box(t, pts[j * 3], pts[j * 3 + 1], pts[j * 3 + 2]);
    }
    return EPNET_OK;
}

extern "C" int epnet_roipool3d_host(const float *pts, const float *boxes3d, const float *pts_feature, float *pooled_pts,
                                    float *pooled_features, int64_t *pooled_empty_flag, int64_t boxes_num,
                                    int64_t pts_num, int64_t feature_len, int64_t sampled_pts_num) {
    EPNET_REQUIRE(boxes_num >= 0 && pts_num >= 0 && feature_len >= 0 && sampled_pts_num >= 0);
    if (boxes_num == 0) return EPNET_OK;
    EPNET_REQUIRE(boxes3d && pooled_empty_flag);
    EPNET_REQUIRE(pts_num == 0 || (pts && (pts_feature || feature_len == 0)));
    EPNET_REQUIRE(sampled_pts_num == 0 || (pooled_pts && (pooled_features || feature_len == 0)));
    const int64_t S = sampled_pts_num, C = feature_len;
    for (int64_t i = 0; i < boxes_num; ++i) {
        const BoxTerms t = box_terms(boxes3d + i * 7);
        float *op = pooled_pts + i * S * 3;
        float *of = pooled_features + i * S * C;
        int64_t cnt = 0;
        for (int64_t j = 0; j < pts_num; ++j) {
            if (!pt_in_box(t, pts[j * 3], pts[j * 3 + 1], pts[j * 3 + 2])) continue;
            if (cnt >= S) break;
            memcpy(op + cnt * 3, pts + j * 3, 3 * sizeof(float));
            if (C) memcpy(of + cnt * C, pts_feature + j * C, (size_t)C * sizeof(float));
            ++cnt;
        }
        pooled_empty_flag[i] = (cnt == 0);
        if (cnt > 0)
            for (int64_t j = cnt; j < S; ++j) {  // cyclic duplication, roipool3d.cpp:180-192
                memcpy(op + j * 3, op + (j % cnt) * 3, 3 * sizeof(float));
                if (C) memcpy(of + j * C, of + (j % cnt) * C, (size_t)C * sizeof(float));
            }
    }
    return EPNET_OK;
}

// get_thresholds, eval.py:8-25
extern "C" int epnet_kitti_thresholds_host(const double *matched, int64_t n, int64_t num_gt, int num_sample_pts, double *thresholds,
                                           int capacity, int *count) {
    EPNET_REQUIRE(n >= 0 && num_gt >= 0 && num_sample_pts >= 2 && capacity >= 0 && count);
    EPNET_REQUIRE(n == 0 || matched);
    std::vector<double> scores;
    for (int64_t i = 0; i < n; ++i)
        if (matched[i] == matched[i]) scores.push_back(matched[i]);
    *count = 0;
    if (scores.empty()) return EPNET_OK;
    EPNET_REQUIRE(num_gt > 0 && (capacity == 0 || thresholds));
    std::sort(scores.begin(), scores.end(), [](double a, double b) { return a > b; });
    const int64_t m = (int64_t)scores.size();
    double current_recall = 0;
    int k = 0;
    for (int64_t i = 0; i < m; ++i) {
        const double l_recall = (double)(i + 1) / (double)num_gt;
        const double r_recall = i < m - 1 ? (double)(i + 2) / (double)num_gt : l_recall;
        if ((r_recall - current_recall) < (current_recall - l_recall) && i < m - 1) continue;
        if (k >= capacity) return EPNET_ENOMEM;
        thresholds[k++] = scores[i];
        current_recall += 1 / (num_sample_pts - 1.0);
    }
    *count = k;
    return EPNET_OK;
}
