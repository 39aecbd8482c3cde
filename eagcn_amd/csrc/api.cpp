// Library-level pieces of the C ABI: version, error string; the entry points of agree.hip (argument checks in front of its launchers).
#include <hip/hip_runtime_api.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/eagcn_hip.h"

namespace eagcn {
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- per-kernel-class timing ---------------------------------------------------------------------
enum { PROF_NTAGS = 9 };
static const char* kTagNames[PROF_NTAGS] = {"index", "pack", "gemm", "agg", "bn", "edge", "readout", "head", "gemm_pair"};
struct ProfRec { hipEvent_t a, b; };
struct ProfState {
    bool on = false;
    std::vector<ProfRec> pool[PROF_NTAGS];
    size_t used[PROF_NTAGS] = {0};
    double work[PROF_NTAGS] = {0};
};
static ProfState g_prof;
bool prof_on() { return g_prof.on; }
void prof_begin(int tag, hipStream_t s, double work) {
    ProfState& p = g_prof;
    if (p.used[tag] == p.pool[tag].size()) {
        ProfRec r;
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
        p.pool[tag].push_back(r);
    }
    p.work[tag] += work;
    (void)hipEventRecord(p.pool[tag][p.used[tag]].a, s);
}
void prof_end(int tag, hipStream_t s) {
    ProfState& p = g_prof;
    if (p.used[tag] >= p.pool[tag].size()) return;
    (void)hipEventRecord(p.pool[tag][p.used[tag]].b, s);
    p.used[tag]++;
}
}  // namespace eagcn

extern "C" void eagcn_prof_enable(int on) { eagcn::g_prof.on = on != 0; }
extern "C" void eagcn_prof_reset(void) {
    for (int t = 0; t < eagcn::PROF_NTAGS; ++t) { eagcn::g_prof.used[t] = 0; eagcn::g_prof.work[t] = 0.0; }
}
extern "C" int eagcn_prof_ntags(void) { return eagcn::PROF_NTAGS; }
extern "C" const char* eagcn_prof_tag_name(int tag) {
    return (tag >= 0 && tag < eagcn::PROF_NTAGS) ? eagcn::kTagNames[tag] : "";
}
/* blocks until the recorded events have completed */
extern "C" int eagcn_prof_read(int tag, double* total_ms, double* work, int64_t* launches) {
    if (tag < 0 || tag >= eagcn::PROF_NTAGS) return -1;
    eagcn::ProfState& p = eagcn::g_prof;
    double ms = 0.0;
    for (size_t i = 0; i < p.used[tag]; ++i) {
        float e = 0.f;
        if (hipEventSynchronize(p.pool[tag][i].b) != hipSuccess) return -2;
        if (hipEventElapsedTime(&e, p.pool[tag][i].a, p.pool[tag][i].b) != hipSuccess) return -2;
        ms += e;
    }
    if (total_ms) *total_ms = ms;
    if (work) *work = p.work[tag];
    if (launches) *launches = (int64_t)p.used[tag];
    return 0;
}

// bumped whenever a struct of include/eagcn_hip.h changes its layout or an entry point its signature (round 4: plane fields of
// eagcn_layer_bufs, eagcn_model.fwd_signal, row capacities of the plane-GEMM entry points); eagcn_amd/_lib.py refuses another version
extern "C" int eagcn_abi_version(void) { return 8; }
/* sizeof() of the ABI structs, so a binding can verify its own struct layout (which: 0 batch,
 * 1 layout, 2 layer_params, 3 layer_bufs, 4 layer_grads) */
extern "C" size_t eagcn_struct_size(int which) {
    switch (which) {
        case 0: return sizeof(eagcn_batch);
        case 1: return sizeof(eagcn_layout);
        case 2: return sizeof(eagcn_layer_params);
        case 3: return sizeof(eagcn_layer_bufs);
        case 4: return sizeof(eagcn_layer_grads);
        case 5: return sizeof(eagcn_head_params);
        case 6: return sizeof(eagcn_head_grads);
        case 7: return sizeof(eagcn_model);
        case 8: return sizeof(eagcn_gat_params);
        case 9: return sizeof(eagcn_pool_att);
        case 10: return sizeof(eagcn_step_loss);
        default: return 0;
    }
}
extern "C" const char* eagcn_last_error(void) { return eagcn::g_err; }

// ---- agreement / thresholded metrics of an evaluation (agree.hip) ---------------------------------
namespace eagcn {
// as kernels.h declares them (this file is plain C++ and does not include the device helpers of common.h)
size_t agree_workspace_bytes(int64_t rows, int T);
int agree_splits(int64_t rows, int T);
int64_t agree_tiles(int64_t rows);
int launch_agree_reg(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T, void* workspace, double* out,
                     hipStream_t s);
int launch_agree_class(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T, float threshold,
                       void* workspace, double* out, hipStream_t s);

#define AGREE_CHECK_ARG(cond, ...)          \
    do {                                    \
        if (!(cond)) {                      \
            ::eagcn::set_error(__VA_ARGS__); \
            return EAGCN_ERR_ARG;           \
        }                                   \
    } while (0)

static int agree_check(const char* fn, const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T,
                       const void* workspace, size_t workspace_bytes, const double* out) {
    AGREE_CHECK_ARG(scores, "%s: scores is null", fn);
    AGREE_CHECK_ARG(targets, "%s: targets is null", fn);
    AGREE_CHECK_ARG(valid, "%s: valid is null", fn);
    AGREE_CHECK_ARG(workspace, "%s: workspace is null", fn);
    AGREE_CHECK_ARG(out, "%s: out is null", fn);
    AGREE_CHECK_ARG(rows >= 1, "%s: rows = %lld, an evaluation needs at least one", fn, (long long)rows);
    AGREE_CHECK_ARG(T >= 1 && T <= 65535, "%s: T = %d is not in 1 .. 65535", fn, T);
    AGREE_CHECK_ARG(rows < (int64_t(1) << 31), "%s: rows = %lld does not fit the 32-bit counters (rows < 2^31)", fn, (long long)rows);
    AGREE_CHECK_ARG(agree_tiles(rows) * T < (int64_t(1) << 31), "%s: rows x T = %lld x %d is more than one launch takes", fn,
                    (long long)rows, T);
    AGREE_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", fn);
    AGREE_CHECK_ARG(workspace_bytes >= agree_workspace_bytes(rows, T), "%s: workspace too small (%zu < %zu bytes)", fn, workspace_bytes,
                    agree_workspace_bytes(rows, T));
    return EAGCN_OK;
}
}  // namespace eagcn

extern "C" size_t eagcn_eval_agreement_workspace_bytes(int64_t rows, int T) {
    return rows < 1 || T < 1 ? 0 : eagcn::agree_workspace_bytes(rows, T);
}
extern "C" int eagcn_eval_agreement_splits(int64_t rows, int T) { return rows < 1 || T < 1 ? 0 : eagcn::agree_splits(rows, T); }

extern "C" int eagcn_eval_reg_agreement(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T,
                                        void* workspace, size_t workspace_bytes, double* out, void* stream) {
    if (int rc = eagcn::agree_check("eagcn_eval_reg_agreement", scores, targets, valid, rows, T, workspace, workspace_bytes, out)) return rc;
    return eagcn::launch_agree_reg(scores, targets, valid, rows, T, workspace, out, (hipStream_t)stream);
}

extern "C" int eagcn_eval_class_threshold(const float* scores, const float* targets, const uint8_t* valid, int64_t rows, int T,
                                          float threshold, void* workspace, size_t workspace_bytes, double* out, void* stream) {
    if (int rc = eagcn::agree_check("eagcn_eval_class_threshold", scores, targets, valid, rows, T, workspace, workspace_bytes, out)) return rc;
    AGREE_CHECK_ARG(threshold == threshold, "eagcn_eval_class_threshold: threshold is NaN");
    return eagcn::launch_agree_class(scores, targets, valid, rows, T, threshold, workspace, out, (hipStream_t)stream);
}
