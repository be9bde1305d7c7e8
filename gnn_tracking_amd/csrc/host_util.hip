// What host_util.h declares and every unit of libgnntrk.so shares: the thread-local last-error string,
// the argument and launch checks, the device query - and the three C entries (include/gnntrk.h) that
// belong to no unit.  Every other entry is defined in the unit that does its work.  No kernels here.
#include <stdio.h>
#include <string.h>

#include "host_util.h"

// ABI layout guards: gnn_tracking_amd/_capi.py mirrors these structs with ctypes
static_assert(sizeof(gnntrk_seg) == 32, "gnntrk_seg layout");
static_assert(sizeof(gnntrk_mlp) == 64, "gnntrk_mlp layout");
static_assert(sizeof(gnntrk_mlp_fwd_args) == 448, "gnntrk_mlp_fwd_args layout");
static_assert(sizeof(gnntrk_mlp_bwd_args) == 808, "gnntrk_mlp_bwd_args layout");
static_assert(sizeof(gnntrk_graph_index) == 72, "gnntrk_graph_index layout");
static_assert(sizeof(gnntrk_graph_index_carry) == 48, "gnntrk_graph_index_carry layout");
static_assert(sizeof(gnntrk_resfcnn) == 8 * (5 + 2 * GNNTRK_RESFCNN_MAX_HIDDEN) + 32, "gnntrk_resfcnn layout");
static_assert(sizeof(gnntrk_efmlp) == 8 * (2 + GNNTRK_RESFCNN_MAX_HIDDEN) + 24 && sizeof(gnntrk_edge_rows) == 56, "gnntrk_efmlp layout");
static_assert(sizeof(gnntrk_resfcnn_grads) == 8 * (5 + 2 * GNNTRK_RESFCNN_MAX_HIDDEN), "gnntrk_resfcnn_grads layout");
static_assert(sizeof(gnntrk_hinge_args) == 56, "gnntrk_hinge_args layout");

namespace gnntrk {

static thread_local char g_err[512] = "";

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg ? msg : "");
    return code;
}

int check_count_i30(const char *entry, const char *what, int64_t n) {
    char msg[160];
    if (n < 0) {
        snprintf(msg, sizeof(msg), "%s: negative %s count", entry, what);
        return fail(GNNTRK_EINVAL, msg);
    }
    if (n >= (int64_t(1) << 30)) {
        snprintf(msg, sizeof(msg), "%s: %lld %ss; at most 2^30-1", entry, (long long)n, what);
        return fail(GNNTRK_EUNSUPPORTED, msg);
    }
    return GNNTRK_OK;
}

int check_workspace(const char *entry, const void *workspace, size_t have, size_t need) {
    if (workspace && have >= need) return GNNTRK_OK;
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: workspace of %zu bytes, need %zu (gnntrk_%s_workspace_bytes)", entry, have, need,
             entry);
    return fail(GNNTRK_EINVAL, msg);
}

int check_hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return GNNTRK_OK;
    const char *s = hipGetErrorString(e);
    const bool oom = s && (strstr(s, "out of memory") || strstr(s, "OutOfMemory"));
    // utils/oom.py:12-18 of the reference looks for "out of memory" in the message
    snprintf(g_err, sizeof(g_err), "%s: HIP error: %s%s", what, s ? s : "?",
             oom ? " (HIP out of memory)" : "");
    return oom ? GNNTRK_ENOMEM : GNNTRK_EHIP;
}

int check_launch(const char *what) { return check_hip(hipGetLastError(), what); }

int cu_count() {
    static thread_local int cached = 0;
    if (cached > 0) return cached;
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
        n = 256;
    cached = n;
    return n;
}

}  // namespace gnntrk

using namespace gnntrk;

extern "C" {

int gnntrk_version(void) { return GNNTRK_VERSION; }
const char *gnntrk_last_error(void) { return g_err; }
int gnntrk_device_cu_count(void) { return cu_count(); }

}  // extern "C"
