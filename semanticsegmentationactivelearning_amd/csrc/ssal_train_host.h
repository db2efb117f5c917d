// ssal_train_host.h -- the steps every training entry of the C ABI shares (ssal_api.hip: ENet's six depths; ssal_icnet_api.hip:
// ICNet's four): what a call is given, the argument checks in their fixed order, the workspace check and the confusion-matrix
// bracket around the launches.  Host C++ only.
#pragma once
#include "../../include/ssal_enet.h"
#include "ssal_confusion.h"
#include "ssal_host.h"
#include "ssal_internal.h"

namespace ssal {

// what every entry is given besides its inputs and parameters: targets, the loss' knobs, outputs, workspace, stream
struct CallArgs {
    const uint8_t *labels;
    const float *mask;
    float weight, label_smoothing;
    double *loss;
    float *grad;
    void *ws;
    int64_t ws_bytes;
    hipStream_t s;
};

// the semi-supervised side of a call as the public entries take it (DESIGN.md sections 16 and 19); NULL = the plain step
struct SemiArgs {
    const uint8_t *labelled;
    int measure;
    float threshold;
    int64_t *confusion, *pseudo_pixels;
    bool with_raw;
};

// the dims of a gradient call whose grid the caller may cap (ICNet's depths): fits = the depth's own limit at these dims,
// noun = what the message calls its kernels ("head gradient kernel's", "fusion gradient kernels'", ...)
inline bool capped_dims_ok(int n, int classes, bool fits) { return n > 0 && classes >= 2 && classes <= 32 && fits; }

inline int capped_dims_check(int n, int h, int w, int classes, int max_workgroups, bool fits, const char *noun)
{
    if (n <= 0) return fail(SSAL_EINVAL, "bad dims n=%d h=%d w=%d", n, h, w);
    if (classes < 2 || classes > 32) return fail(SSAL_EINVAL, "classes must be in [2,32] (got %d)", classes);
    if (max_workgroups < 0) return fail(SSAL_EINVAL, "max_workgroups must be >= 0 (got %d)", max_workgroups);
    if (!fits) return fail(SSAL_EINVAL, "feature map %dx%d (n=%d) is beyond the %s limit", h, w, n, noun);
    return SSAL_OK;
}

// the semi arguments, then the pointers (`inputs`: the entry's own features / frames / parameters, and-ed); a semi call's
// label and mask planes may be NULL when no image is labelled
inline int args_check(bool inputs, const CallArgs &a, const SemiArgs *semi)
{
    if (semi && (semi->measure < 0 || semi->measure > 2))
        return fail(SSAL_ENOTIMPL, "Uncertainty function not implemented (measure=%d)", semi->measure);
    if (semi && !semi->labelled && (!a.labels || !a.mask))
        return fail(SSAL_EINVAL, "labels_dev / mask_dev may be NULL only when labelled_dev marks no image as labelled");
    if (!inputs || !a.loss || !a.grad || !a.ws || (!semi && (!a.labels || !a.mask)))
        return fail(SSAL_EINVAL, "NULL device pointer");
    return SSAL_OK;
}

// judged once the call's pieces are carved from b (pointer arithmetic only), before anything is launched
inline int ws_check(int64_t need, const Bump &b, const CallArgs &a)
{
    if (a.ws_bytes < need) return fail(SSAL_ENOMEM, "workspace too small: need %lld bytes, got %lld", (long long)need,
                                       (long long)a.ws_bytes);
    return b.ok ? SSAL_OK : fail(SSAL_ENOMEM, "workspace too small: need %lld bytes", (long long)need);
}

// a features entry has its features already: nothing to run where an images entry runs the trunk
inline int no_trunk(bool) { return SSAL_OK; }

// launches(rep, reps) with the confusion replicas zeroed before and folded into the caller's matrix after it; without a
// matrix (a plain call, or a semi call that asks for none) rep is NULL and neither the memset nor the fold is issued
template <typename Launches>
int with_confusion(unsigned long long *rep, int classes, int64_t *confusion_dev, hipStream_t s, Launches launches)
{
    const int reps = knobs().conf_reps;
    if (confusion_dev) HIP_TRY(hipMemsetAsync(rep, 0, (size_t)reps * conf_rep_stride(classes * classes) * 8, s));
    if (int rc = launches(confusion_dev ? rep : nullptr, reps)) return rc;
    if (confusion_dev) HIP_TRY(launch_confusion_fold(rep, reps, classes, confusion_dev, s));
    return SSAL_OK;
}

}  // namespace ssal
