// ssal_icnet_api.hip -- the C ABI of the ICNet row (include/ssal_icnet.h): handle, weight staging, layer
// sequencing of ICNET_SPEC.md.  Host C++ only; no torch types.  gfx950 (MI355X) only.
#include "../../include/ssal_enet.h"
#include "../../include/ssal_icnet.h"
#include "ssal_bf16x3.h"
#include "ssal_bottleneck_args.h"
#include "ssal_confusion.h"
#include "ssal_host.h"
#include "ssal_icnet.h"
#include "ssal_internal.h"
#include "ssal_prof.h"
#include "ssal_train_host.h"
#include "ssal_train_icnet.h"
#include "ssal_train_icnet_cascade.h"
#include "ssal_train_icnet_fusion.h"
#include "ssal_train_icnet_highres.h"
#include "ssal_train_icnet_bneck.h"
#include "ssal_train_icnet_bneck2.h"
#include "ssal_train_icnet_pool.h"
#include "ssal_train_icnet_pyramid.h"

#include <math.h>

#include <map>
#include <set>
#include <string>
#include <vector>

using namespace ssal;

namespace {

// ---- topology (ICNET_SPEC.md sections 1-4) -----------------------------------------------------------
struct ConvSpec {
    std::string name;
    int k, cin, cout, stride, dil;
    bool bn;  // false: conv6_cls (bias instead)
};

struct BneckSpec {
    const char *name;
    int cin, mid, cout, stride, dil;
    bool proj;
};

const BneckSpec kBnecks[] = {
    {"conv2_1", 64, 32, 128, 1, 1, true},     {"conv2_2", 128, 32, 128, 1, 1, false},
    {"conv2_3", 128, 32, 128, 1, 1, false},   {"conv3_1", 128, 64, 256, 2, 1, true},
    {"conv3_2", 256, 64, 256, 1, 1, false},   {"conv3_3", 256, 64, 256, 1, 1, false},
    {"conv3_4", 256, 64, 256, 1, 1, false},   {"conv4_1", 256, 128, 512, 1, 2, true},
    {"conv4_2", 512, 128, 512, 1, 2, false},  {"conv4_3", 512, 128, 512, 1, 2, false},
    {"conv4_4", 512, 128, 512, 1, 2, false},  {"conv4_5", 512, 128, 512, 1, 2, false},
    {"conv4_6", 512, 128, 512, 1, 2, false},  {"conv5_1", 512, 256, 1024, 1, 4, true},
    {"conv5_2", 1024, 256, 1024, 1, 4, false}, {"conv5_3", 1024, 256, 1024, 1, 4, false},
};
const int kNumBnecks = (int)(sizeof(kBnecks) / sizeof(kBnecks[0]));
const int kStemBnecks = 4;  // conv2_1 .. conv3_1 run on the shared 1/2-image stem

std::vector<ConvSpec> conv_specs(int c_in, int classes)
{
    std::vector<ConvSpec> L;
    auto conv = [&](const std::string &n, int k, int cin, int cout, int s = 1, int d = 1, bool bn = true) {
        L.push_back({n, k, cin, cout, s, d, bn});
    };
    conv("conv1_1_3x3_s2", 3, c_in, 32, 2);
    conv("conv1_2_3x3", 3, 32, 32);
    conv("conv1_3_3x3", 3, 32, 64);
    for (int i = 0; i < kNumBnecks; ++i) {
        const BneckSpec &b = kBnecks[i];
        const std::string n = b.name;
        conv(n + "_1x1_reduce", 1, b.cin, b.mid, b.stride);
        conv(n + "_3x3", 3, b.mid, b.mid, 1, b.dil);
        conv(n + "_1x1_increase", 1, b.mid, b.cout);
        if (b.proj) conv(n + "_1x1_proj", 1, b.cin, b.cout, b.stride);
    }
    conv("conv5_4_k1", 1, 1024, 256);
    conv("conv_sub4", 3, 256, 128, 1, 2);
    conv("conv3_1_sub2_proj", 1, 256, 128);
    conv("conv_sub2", 3, 128, 128, 1, 2);
    conv("conv1_sub1", 3, c_in, 32, 2);
    conv("conv2_sub1", 3, 32, 32, 2);
    conv("conv3_sub1", 3, 32, 64, 2);
    conv("conv3_sub1_proj", 1, 64, 128);
    conv("conv6_cls", 1, 128, classes, 1, 1, false);
    return L;
}

struct ConvDev {
    ConvSpec spec;
    const float *w = nullptr;      // igemm layout (cin % 32 == 0) or raw HWIO (first convs)
    const float *scale = nullptr;  // [CoutP]
    const float *shift = nullptr;  // [CoutP]
    const float *w_hwio = nullptr; // plain HWIO copy: only the layers of the blocks in fused_bneck() (else NULL)
    const float *wq = nullptr;     // on the *_1x1_reduce layer of a fused_bneck() block: its three kernels in quad layout (bnk_quad_layout)
    const float *w3 = nullptr;     // cin % 32 == 0: the kernel pre-split for k_igemm_bf16x3 (bf16x3::pack_igemm), next to w
    const float *pk3 = nullptr;    // on the *_1x1_reduce layer of a fused_bneck() block: bf16x3::pack_layer of its three kernels
};

// identity-shortcut bottlenecks with ENet's stage-2 shape (128 -> 32 -> 3x3 -> 128 on the 1/8-resolution map): the score
// path runs them as ONE launch of ENet's fused bottleneck kernel (k_bottleneck_mfma, PReLU slopes = 0 == ReLU); the
// three 1x1-layer launches of the per-layer path read / write 302 MB each at that size and are HBM-bound
bool fused_bneck(const BneckSpec &b) { return !b.proj && b.cin == 128 && b.mid == 32 && b.cout == 128 && b.stride == 1; }

// one materialised activation tensor: spatial divisor relative to the input and channel count
struct ActSpec {
    std::string name;
    int div, c;
};

}  // namespace

struct ssal_icnet {
    int c_in = 3, classes = 19;
    std::vector<ConvSpec> specs;
    std::vector<HostTensor> tensors;
    std::map<std::string, int> index;
    std::map<std::string, ConvDev> convs;
    std::vector<ActSpec> acts;
    float *arena = nullptr;
    size_t arena_floats = 0;
    const float *zeros128 = nullptr;  // PReLU slopes of the fused bottleneck launches (slope 0 == ReLU)
    bool committed = false;
    int device = -1;  // the device the arena lives on (set by commit); calls on another device are refused
};

namespace {

void add_tensor(ssal_icnet *h, const std::string &name, std::vector<int64_t> dims)
{
    HostTensor t;
    t.name = name;
    t.dims = std::move(dims);
    h->index[name] = (int)h->tensors.size();
    h->tensors.push_back(std::move(t));
}

void declare(ssal_icnet *h)
{
    h->specs = conv_specs(h->c_in, h->classes);
    for (const ConvSpec &s : h->specs) {
        add_tensor(h, s.name + ".kernel", {s.k, s.k, s.cin, s.cout});
        if (s.bn) {
            add_tensor(h, s.name + ".mean", {s.cout});
            add_tensor(h, s.name + ".variance", {s.cout});
            add_tensor(h, s.name + ".gamma", {s.cout});
            add_tensor(h, s.name + ".beta", {s.cout});
        } else {
            add_tensor(h, s.name + ".bias", {s.cout});
        }
    }
    // materialised activations, in execution order (each keeps its own buffer: nothing is aliased, so every
    // ICNET_SPEC layer output of the last call can be inspected through ssal_icnet_endpoint_info)
    auto act = [&](const std::string &n, int div, int c) { h->acts.push_back({n, div, c}); };
    act("conv1_1_3x3_s2", 4, 32);
    act("conv1_2_3x3", 4, 32);
    act("conv1_3_3x3", 4, 64);
    act("pool1_3x3_s2", 8, 64);
    int div = 8;
    for (int i = 0; i < kNumBnecks; ++i) {
        const BneckSpec &b = kBnecks[i];
        if (i == kStemBnecks) {
            act("conv3_1_sub4", 32, 256);
            div = 32;
        }
        const int odiv = div * b.stride;
        const std::string n = b.name;
        act(n + "_1x1_reduce", odiv, b.mid);
        act(n + "_3x3", odiv, b.mid);
        if (b.proj) act(n + "_1x1_proj", odiv, b.cout);
        act(n, odiv, b.cout);
        div = odiv;
    }
    act("conv5_3_sum", 32, 1024);
    act("conv5_4_k1", 32, 256);
    act("conv1_sub1", 2, 32);
    act("conv2_sub1", 4, 32);
    act("conv3_sub1", 8, 64);
    act("conv3_1_sub2_proj", 16, 128);
    act("sub24_sum", 16, 128);
    act("conv3_sub1_proj", 8, 128);
    act("sub12_sum", 8, 128);
    act("conv6_cls", 4, h->classes);
}

const std::vector<float> &T(const ssal_icnet *h, const std::string &name) { return h->tensors[h->index.at(name)].data; }

struct IcWorkspace {
    std::map<std::string, float *> act;
    float *pooled = nullptr;
    double *partial = nullptr;
    int64_t bytes = 0;
    bool ok = true;
};

IcWorkspace carve(const ssal_icnet *net, void *ws, int64_t ws_bytes, int64_t n, int64_t h, int64_t w)
{
    Bump b(ws, ws_bytes);
    IcWorkspace W;
    for (const ActSpec &a : net->acts) {
        W.act[a.name] = b.take<float>(n * (h / a.div) * (w / a.div) * a.c);
    }
    W.pooled = b.take<float>(ppm_scratch_floats((int)n, (int)(h / 32), 1024));
    W.partial = b.take<double>(n * (int64_t)upscore_blocks((int)(h / 4), (int)(w / 4)));
    W.bytes = b.off;
    W.ok = b.ok;
    return W;
}

int check_dims(const ssal_icnet *net, int n, int h, int w)
{
    if (!net) return fail(SSAL_EINVAL, "net is NULL");
    if (!net->committed) return fail(SSAL_ESTATE, "ssal_icnet_commit() has not been called");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != net->device)
        return fail(SSAL_ESTATE, "the handle was committed on device %d but the current device is %d (one handle per device)",
                    net->device, dev);
    if (n <= 0 || h <= 0 || w <= 0) return fail(SSAL_EINVAL, "bad dims n=%d h=%d w=%d", n, h, w);
    if (h % 32 || w % 32) return fail(SSAL_EINVAL, "ICNet needs H and W divisible by 32 (got %dx%d)", h, w);
    // the convolution kernels address each tensor with 32-bit byte offsets; the largest one (conv1_sub1's output) holds
    // n*h*w/4 pixels x 32 floats = 32 bytes per input pixel
    if ((int64_t)n * h * w >= ((int64_t)1 << 27)) return fail(SSAL_EINVAL, "batch too large (n=%d h=%d w=%d): split it", n, h, w);
    return SSAL_OK;
}

#define HIP_RET(expr)                    \
    do {                                 \
        hipError_t e_ = (expr);          \
        if (e_ != hipSuccess) return e_; \
    } while (0)

// conv -> BN -> [+res] -> [relu] on the matrix cores
hipError_t run_conv(const ssal_icnet *net, const std::string &name, const float *x, int n, int h, int w,
                    const float *res, bool relu, bool up2, float *y, hipStream_t s, int arith = SSAL_ARITH_F32)
{
    const ConvDev &c = net->convs.at(name);
    return launch_igemm(x, n, h, w, c.spec.cin, c.w, c.spec.k, c.spec.k, c.spec.cout, c.spec.stride, c.spec.dil,
                        c.scale, c.shift, res, relu, up2, y, s, arith, c.w3);
}

// runs everything up to the 1/4-resolution class logits (ICNET_SPEC conv6_cls)
// one chain of the image-group schedule: a contiguous range of the batch with its views of the workspace and its stream
struct Grp {
    IcWorkspace W;
    const void *x;
    int n;
    hipStream_t s;
    float *A(const std::string &nm) const { return W.act.at(nm); }
};

// fused: the score path (nobody reads the intermediate layer outputs) may run a whole block as one launch; the forward
// path keeps one launch per ICNET_SPEC layer, so that every layer output of the last forward call is an endpoint.
// Every layer is issued for all groups before the next layer (layer-major order: the chains advance together on their
// streams instead of one chain's 70 launches queueing up in front of the other's).
// written != NULL: DRY run -- nothing is launched, the names of the activation buffers this schedule would write are
// collected instead (ssal_icnet_endpoint_valid_after_score: the one place that knows which layer outputs a fused launch
// swallows is the schedule itself)
// head = false: the schedule ends at sub12_sum (the output-layer trainer runs conv6_cls on the weights it trains)
// fusion = false (with head = false): it ends at sub24_sum and conv3_sub1 (the fusion trainer runs the last fusion block too)
// cascade = false (with fusion = false): it ends once conv5_4_k1, conv3_1 and conv3_sub1 are written (the cascade trainer runs
// both fusion blocks; every fused launch above writes those three: none of them is swallowed)
// highres = false (with cascade = false): the high-resolution branch is left out too -- only the two backbone branches run
// (the high-resolution trainer runs conv1_sub1 .. conv3_sub1 on the weights it trains)
// k1 = false (with cascade = false): the low-resolution schedule ends after the launch that writes conv5_3_sum -- conv5_4_k1 is
// neither launched nor written (the pyramid trainer runs it on the weights it trains); the high-resolution branch still runs
// increase = false (implies k1 = false): the low-resolution schedule ends inside conv5_3 -- conv5_1 and conv5_2 run as ever, conv5_3's
// 1x1_reduce and 3x3 run as the separate run_conv launches they always are at 1024 channels (fused_bneck() is the 128-channel
// family) and write conv5_3_1x1_reduce and conv5_3_3x3; its increase layer, launch_ppm and conv5_4_k1 are neither launched nor
// written (the pooling trainer runs them on the weights it trains); the high-resolution branch still runs
// reduce = false (implies increase = false): the low-resolution schedule ends after the launch that writes conv5_2 -- conv5_3's
// 1x1_reduce and 3x3 are neither launched nor written either (the bottleneck trainer runs the whole of conv5_3 on the weights it
// trains); the high-resolution branch still runs
// block2 = false (implies reduce = false): the low-resolution schedule ends after the launch that writes conv5_1 -- no layer of
// conv5_2 is launched or written either (the deep bottleneck trainer runs conv5_2 and conv5_3 on the weights it trains); the
// high-resolution branch still runs
// arith: SSAL_ARITH_BF16X3 hands the mode to every run_conv (launch_igemm keeps what has no split kernel exact) and runs the
// fused blocks on ENet's bf16x3 regular-block kernel; the training, evaluate and regions entries pass the default
hipError_t run_trunk(const ssal_icnet *net, std::vector<Grp> &grp, bool x_is_u8, int h, int w, bool fused,
                     std::set<std::string> *written = nullptr, bool head = true, bool fusion = true, bool cascade = true,
                     bool highres = true, int arith = SSAL_ARITH_F32, bool k1 = true, bool increase = true,
                     bool reduce = true, bool block2 = true)
{
    if (!block2) reduce = false;  // a schedule that ends in front of conv5_2 writes no conv5_2 for conv5_3's reduce layer to read
    if (!reduce) increase = false;  // a schedule that ends in front of conv5_3 writes no conv5_3_3x3 for the increase layer to read
    if (!increase) k1 = false;  // a schedule that ends inside conv5_3 writes no conv5_3_sum for conv5_4_k1 to read
    const bool dry = written != nullptr;
#define OUT(name) do { if (dry) written->insert(name); } while (0)
#define EACH(expr)                                     \
    for (Grp & q : grp) {                              \
        if (dry) break;                                \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) return e_;               \
    }
    // ---- medium-resolution branch / shared stem (section 1) ----
    // fused score path: the first two convolutions of a branch in one launch (k_front2), the first one's output never
    // reaches HBM (and is no endpoint of such a call)
    const int front = fused && ssal::mfma_family() ? ssal::knobs().ic_front : 0;
    if ((front & 2) && front2_supported(h, w, net->c_in, 2, 1)) {
        const ConvDev &c = net->convs.at("conv1_1_3x3_s2"), &c2 = net->convs.at("conv1_2_3x3");
        OUT("conv1_2_3x3");
        EACH(launch_front2(q.x, x_is_u8, q.n, h, w, net->c_in, 2, c.w, c.scale, c.shift, c2.w, c2.scale, c2.shift, 1,
                           q.A("conv1_2_3x3"), q.s));
    } else {
        const ConvDev &c = net->convs.at("conv1_1_3x3_s2");
        OUT("conv1_1_3x3_s2");
        OUT("conv1_2_3x3");
        EACH(launch_conv_first(q.x, x_is_u8, q.n, h, w, net->c_in, 2, c.w, c.scale, c.shift, q.A("conv1_1_3x3_s2"), q.s));
        EACH(run_conv(net, "conv1_2_3x3", q.A("conv1_1_3x3_s2"), q.n, h / 4, w / 4, nullptr, true, false, q.A("conv1_2_3x3"), q.s, arith));
    }
    OUT("conv1_3_3x3");
    OUT("pool1_3x3_s2");
    EACH(run_conv(net, "conv1_3_3x3", q.A("conv1_2_3x3"), q.n, h / 4, w / 4, nullptr, true, false, q.A("conv1_3_3x3"), q.s, arith));
    EACH(launch_maxpool3x3_s2(q.A("conv1_3_3x3"), q.n, h / 4, w / 4, 64, q.A("pool1_3x3_s2"), q.s));
    std::string cur = "pool1_3x3_s2";
    int ch = h / 8, cw = w / 8;
    for (int i = 0; i < kNumBnecks; ++i) {
        const BneckSpec &b = kBnecks[i];
        const std::string nm = b.name;
        if (!reduce && i == kNumBnecks - 1) break;  // conv5_3 of a schedule that ends behind conv5_2
        if (!block2 && i == kNumBnecks - 2) break;  // conv5_2 of a schedule that ends behind conv5_1
        if (i == kStemBnecks) {
            // section 2: conv3_1_sub4 = resize_bilinear(conv3_1, 1/2)
            OUT("conv3_1_sub4");
            EACH(launch_resize_bilinear(q.A(cur), q.n, ch, cw, 256, ch / 2, cw / 2, q.A("conv3_1_sub4"), q.s));
            cur = "conv3_1_sub4";
            ch /= 2;
            cw /= 2;
        }
        const int oh = ch / b.stride, ow = cw / b.stride;
        if (fused && ssal::mfma_family() && fused_bneck(b) && b.dil >= 1) {
            // reduce -> 3x3 -> increase + identity shortcut -> ReLU == ENet's regular bottleneck with zero slopes: same
            // (kh, kw, ci)-ascending fmaf chains, same folded batch-norm, same `fmaf(e, s, t) + x` merge; a ReLU written as
            // PReLU(slope 0) yields -0.0 where max(v, 0) yields +0.0, which no later layer can tell apart (every consumer
            // adds it into a +0-initialised chain)
            const ConvDev &r = net->convs.at(nm + "_1x1_reduce"), &c3 = net->convs.at(nm + "_3x3"),
                          &inc = net->convs.at(nm + "_1x1_increase");
            OUT(nm);
            if (arith == SSAL_ARITH_BF16X3 && r.pk3 && bottleneck_bf16x3_fits(ch, cw)) {  // opt-in: NOT bit-identical
                BnkArgs ba;
                memset(&ba, 0, sizeof(ba));
                ba.wp = r.w_hwio; ba.ps = r.scale; ba.pt = r.shift; ba.pa = net->zeros128;
                ba.wc = c3.w_hwio; ba.cs = c3.scale; ba.ct = c3.shift; ba.ca = net->zeros128;
                ba.we = inc.w_hwio; ba.es = inc.scale; ba.et = inc.shift; ba.ra = net->zeros128;
                ba.H = ch; ba.W = cw; ba.dil = b.dil;
                for (Grp & q : grp) {
                    if (dry) break;
                    ba.x = q.A(cur); ba.y = q.A(nm); ba.N = q.n;
                    HIP_RET(launch_bottleneck_bf16x3(ba, r.pk3, q.s));
                }
                cur = nm;
                continue;
            }
            EACH(launch_bottleneck_mfma(q.A(cur), q.A(nm), q.n, ch, cw, b.cin, b.dil, r.w_hwio, r.scale, r.shift,
                                        net->zeros128, c3.w_hwio, nullptr, c3.scale, c3.shift, net->zeros128, inc.w_hwio,
                                        inc.scale, inc.shift, net->zeros128, q.s, r.wq));
            cur = nm;
            continue;
        }
        std::string shortcut = cur;
        // fused score path (knob ic_dual): the projection shortcut is evaluated inside the increase launch (k_igemm<.., DUAL>)
        // and never reaches HBM
        const bool dual = b.proj && fused && ssal::mfma_family() && ssal::knobs().ic_dual;
        if (b.proj && !dual) {
            OUT(nm + "_1x1_proj");
            EACH(run_conv(net, nm + "_1x1_proj", q.A(cur), q.n, ch, cw, nullptr, false, false, q.A(nm + "_1x1_proj"), q.s, arith));
            shortcut = nm + "_1x1_proj";
        }
        const bool stop = !increase && i == kNumBnecks - 1;  // conv5_3 of a schedule that ends in front of its increase layer
        OUT(nm + "_1x1_reduce");
        OUT(nm + "_3x3");
        if (!stop) OUT(nm);
        EACH(run_conv(net, nm + "_1x1_reduce", q.A(cur), q.n, ch, cw, nullptr, true, false, q.A(nm + "_1x1_reduce"), q.s, arith));
        EACH(run_conv(net, nm + "_3x3", q.A(nm + "_1x1_reduce"), q.n, oh, ow, nullptr, true, false, q.A(nm + "_3x3"), q.s, arith));
        if (stop) break;
        if (dual) {
            const ConvDev &ci_ = net->convs.at(nm + "_1x1_increase"), &cp = net->convs.at(nm + "_1x1_proj");
            EACH(launch_igemm_dual(q.A(nm + "_3x3"), q.n, oh, ow, ci_.spec.cin, ci_.w, ci_.spec.cout, ci_.scale, ci_.shift,
                                   q.A(cur), cp.spec.cin, b.stride, cp.w, cp.scale, cp.shift, true, q.A(nm), q.s));
        } else {
            EACH(run_conv(net, nm + "_1x1_increase", q.A(nm + "_3x3"), q.n, oh, ow, q.A(shortcut), true, false, q.A(nm), q.s, arith));
        }
        cur = nm;
        ch = oh;
        cw = ow;
    }
    // pyramid pooling + conv5_4_k1
    if (increase) OUT("conv5_3_sum");
    if (k1) OUT("conv5_4_k1");
    if (increase) EACH(launch_ppm(q.A(cur), q.n, ch, cw, 1024, q.W.pooled, q.A("conv5_3_sum"), q.s));
    if (k1) EACH(run_conv(net, "conv5_4_k1", q.A("conv5_3_sum"), q.n, ch, cw, nullptr, true, false, q.A("conv5_4_k1"), q.s, arith));
    // ---- high-resolution branch (section 3) ----
    if (!highres) return hipSuccess;
    if ((front & 1) && front2_supported(h, w, net->c_in, 1, 2)) {
        const ConvDev &c = net->convs.at("conv1_sub1"), &c2 = net->convs.at("conv2_sub1");
        OUT("conv2_sub1");
        EACH(launch_front2(q.x, x_is_u8, q.n, h, w, net->c_in, 1, c.w, c.scale, c.shift, c2.w, c2.scale, c2.shift, 2,
                           q.A("conv2_sub1"), q.s));
    } else {
        const ConvDev &c = net->convs.at("conv1_sub1");
        OUT("conv1_sub1");
        OUT("conv2_sub1");
        EACH(launch_conv_first(q.x, x_is_u8, q.n, h, w, net->c_in, 1, c.w, c.scale, c.shift, q.A("conv1_sub1"), q.s));
        EACH(run_conv(net, "conv2_sub1", q.A("conv1_sub1"), q.n, h / 2, w / 2, nullptr, true, false, q.A("conv2_sub1"), q.s, arith));
    }
    OUT("conv3_sub1");
    if (cascade) for (const char *nm_ : {"conv3_1_sub2_proj", "sub24_sum"}) OUT(nm_);
    if (fusion) for (const char *nm_ : {"conv3_sub1_proj", "sub12_sum"}) OUT(nm_);
    if (head) OUT("conv6_cls");
    EACH(run_conv(net, "conv3_sub1", q.A("conv2_sub1"), q.n, h / 4, w / 4, nullptr, true, false, q.A("conv3_sub1"), q.s, arith));
    // ---- cascade feature fusion (section 4): the 2x interpolations are evaluated inside the dilated convs ----
    if (cascade) {
        EACH(run_conv(net, "conv3_1_sub2_proj", q.A("conv3_1"), q.n, h / 16, w / 16, nullptr, false, false,
                      q.A("conv3_1_sub2_proj"), q.s, arith));
        EACH(run_conv(net, "conv_sub4", q.A("conv5_4_k1"), q.n, h / 32, w / 32, q.A("conv3_1_sub2_proj"), true, true,
                      q.A("sub24_sum"), q.s, arith));
    }
    if (fusion) {
        EACH(run_conv(net, "conv3_sub1_proj", q.A("conv3_sub1"), q.n, h / 8, w / 8, nullptr, false, false,
                      q.A("conv3_sub1_proj"), q.s, arith));
        EACH(run_conv(net, "conv_sub2", q.A("sub24_sum"), q.n, h / 16, w / 16, q.A("conv3_sub1_proj"), true, true,
                      q.A("sub12_sum"), q.s, arith));
    }
    // sub12_sum_interp (2x) + conv6_cls (1x1, bias)
    if (head) EACH(run_conv(net, "conv6_cls", q.A("sub12_sum"), q.n, h / 8, w / 8, nullptr, false, true, q.A("conv6_cls"), q.s, arith));
#undef EACH
#undef OUT
    return hipSuccess;
}

int forward_any(ssal_icnet *net, const void *x_dev, bool u8, int n, int h, int w, float *logits_dev, void *ws_dev,
                int64_t ws_bytes, void *stream, int arith = SSAL_ARITH_F32)
{
    int rc = check_dims(net, n, h, w);
    if (rc) return rc;
    if (!x_dev || !logits_dev || !ws_dev) return fail(SSAL_EINVAL, "NULL device pointer");
    IcWorkspace W = carve(net, ws_dev, ws_bytes, n, h, w);
    if (!W.ok) return fail(SSAL_ENOMEM, "workspace too small: need %lld bytes, got %lld", (long long)W.bytes, (long long)ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    std::vector<Grp> one(1);
    one[0] = {W, x_dev, n, s};
    HIP_TRY(run_trunk(net, one, u8, h, w, false, nullptr, true, true, true, true, arith));
    HIP_TRY(launch_resize_bilinear(W.act.at("conv6_cls"), n, h / 4, w / 4, net->classes, h, w, logits_dev, s));
    return SSAL_OK;
}

// The fused trunk of a score-type call (ranking: score_any; validation: eval_any) up to conv6_cls, then tail(chain, first
// image of the chain) on every chain's stream, then the join: one schedule, one set of knobs for both passes.
template <class Tail>
int run_scored(ssal_icnet *net, const void *x_dev, bool u8, int n, int h, int w, const IcWorkspace &W, hipStream_t s, Tail tail,
               int arith = SSAL_ARITH_F32)
{
    // image-group schedule (same knob and same reasoning as ENet's run_net, ssal_api.hip): the batch runs as G chains of
    // ~n / G images on library-owned side streams, forked from / joined into the caller's stream with events
    int G = ssal::knobs().ic_groups;  // ICNet's own chain count (default 1; ENet: img_groups)
    if (G < 2 || G > 8 || n < G || !ssal::mfma_family() || ssal::prof_enabled()) G = 1;
    const int64_t px = (int64_t)h * w, ppm_img = ppm_scratch_floats(1, h / 32, 1024);
    const int blocks = upscore_blocks(h / 4, w / 4);
    std::vector<Grp> grp(G);
    std::vector<int64_t> first(G + 1);
    for (int g = 0; g <= G; ++g) first[g] = (int64_t)g * n / G;
    // fork / join events are private to this call (ssal::ChainSet, ssal_api.hip); a failure half way still joins the chains
    ssal::ChainSet cs;
    if (G > 1) HIP_TRY(cs.begin(G, s));
    for (int g = 0; g < G; ++g) {
        const int64_t i0 = first[g];
        Grp &q = grp[g];
        q.W = W;
        for (const ActSpec &a : net->acts) q.W.act[a.name] = W.act.at(a.name) + i0 * (h / a.div) * (w / a.div) * a.c;
        q.W.pooled = W.pooled + i0 * ppm_img;
        q.W.partial = W.partial + i0 * blocks;
        q.x = (const char *)x_dev + (size_t)i0 * px * net->c_in * (u8 ? 1 : 4);
        q.n = (int)(first[g + 1] - i0);
        q.s = s;
        if (G > 1) q.s = cs.side[g];
    }
    set_launch_concurrency(G);
    const hipError_t trunk_rc = run_trunk(net, grp, u8, h, w, true, nullptr, true, true, true, true, arith);
    set_launch_concurrency(1);
    HIP_TRY(trunk_rc);
    for (int g = 0; g < G; ++g) HIP_TRY(tail(grp[g], first[g]));
    HIP_TRY(cs.end());
    return SSAL_OK;
}

int score_any(ssal_icnet *net, const void *x_dev, bool u8, int n, int h, int w, int measure, float threshold,
              double *scores_dev, uint8_t *label_dev, uint8_t *mask_dev, float *conf_dev, void *ws_dev,
              int64_t ws_bytes, void *stream, int arith = SSAL_ARITH_F32)
{
    int rc = check_dims(net, n, h, w);
    if (rc) return rc;
    if (measure < 0 || measure > 2) return fail(SSAL_ENOTIMPL, "Uncertainty function not implemented (measure=%d)", measure);
    if (!x_dev || !scores_dev || !ws_dev) return fail(SSAL_EINVAL, "NULL device pointer");
    if (((uintptr_t)label_dev | (uintptr_t)mask_dev) & 3 || ((uintptr_t)conf_dev & 15))
        return fail(SSAL_EINVAL, "label_dev / mask_dev must be 4-byte aligned and conf_dev 16-byte aligned");
    IcWorkspace W = carve(net, ws_dev, ws_bytes, n, h, w);
    if (!W.ok) return fail(SSAL_ENOMEM, "workspace too small: need %lld bytes, got %lld", (long long)W.bytes, (long long)ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    const int64_t px = (int64_t)h * w;
    if ((rc = run_scored(net, x_dev, u8, n, h, w, W, s, [&](const Grp &q, int64_t i0) {
            return launch_upscore(q.A("conv6_cls"), q.n, h / 4, w / 4, net->classes, measure, threshold, q.W.partial,
                                  label_dev ? label_dev + i0 * px : nullptr, mask_dev ? mask_dev + i0 * px : nullptr,
                                  conf_dev ? conf_dev + i0 * px : nullptr, q.s);
        }, arith)))
        return rc;
    HIP_TRY(launch_reduce_mean(W.partial, n, upscore_blocks(h / 4, w / 4), (double)h * (double)w, scores_dev, s));
    return SSAL_OK;
}

// ---- evaluation pass: the score path's trunk, then conv6_interp + argmax + confusion matrix in one launch (k_upeval) ----
int64_t conf_replica_bytes(int classes) { return (int64_t)ssal::kConfMaxReps * ssal::conf_rep_stride(classes * classes) * 8; }

int64_t eval_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    if (!net || !net->committed || n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32) return -1;
    if (net->classes < 2 || net->classes > ssal::kConfMaxClasses) return -1;
    const IcWorkspace W = carve(net, nullptr, 0, n, h, w);
    return (W.bytes + 255) / 256 * 256 + conf_replica_bytes(net->classes) + 256;
}

int eval_any(ssal_icnet *net, const void *x_dev, bool u8, int n, int h, int w, const uint8_t *labels_dev,
             const uint8_t *mask_dev, int64_t *confusion_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    int rc = check_dims(net, n, h, w);
    if (rc) return rc;
    const int K = net->classes;
    if (K < 2 || K > ssal::kConfMaxClasses) return fail(SSAL_EINVAL, "classes must be in [2,32] (got %d)", K);
    if (!x_dev || !labels_dev || !confusion_dev || !ws_dev) return fail(SSAL_EINVAL, "NULL device pointer");
    if (((uintptr_t)labels_dev | (uintptr_t)mask_dev) & 3)
        return fail(SSAL_EINVAL, "labels_dev / mask_dev must be 4-byte aligned");
    const int64_t need = eval_workspace_bytes(net, n, h, w);
    IcWorkspace W = carve(net, ws_dev, ws_bytes, n, h, w);
    if (!W.ok || ws_bytes < need)
        return fail(SSAL_ENOMEM, "workspace too small: need %lld bytes, got %lld", (long long)need, (long long)ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    const int reps = ssal::knobs().conf_reps;
    unsigned long long *rep = (unsigned long long *)((char *)ws_dev + (W.bytes + 255) / 256 * 256);
    HIP_TRY(hipMemsetAsync(rep, 0, (size_t)reps * ssal::conf_rep_stride(K * K) * 8, s));  // before the chains fork from s
    const int64_t px = (int64_t)h * w;
    if ((rc = run_scored(net, x_dev, u8, n, h, w, W, s, [&](const Grp &q, int64_t i0) {
            return launch_upeval(q.A("conv6_cls"), q.n, h / 4, w / 4, K, labels_dev + i0 * px,
                                 mask_dev ? mask_dev + i0 * px : nullptr, rep, reps, q.s);
        })))
        return rc;
    HIP_TRY(launch_confusion_fold(rep, reps, K, confusion_dev, s));
    return SSAL_OK;
}

// folded batch-norm (extra_ops.py:181-184, eps 1e-3) padded to CoutP entries
void fold_bn_padded(const float *mean, const float *var, const float *gamma, const float *beta, const float *bias,
                    int c, std::vector<float> &s, std::vector<float> &t)
{
    const int cp = (c + 31) / 32 * 32;
    s.assign(cp, 0.0f);
    t.assign(cp, 0.0f);
    for (int i = 0; i < c; ++i) {
        if (mean) {
            const float sg = gamma[i] / sqrtf(var[i] + 1e-3f);
            s[i] = sg;
            t[i] = fmaf(-mean[i], sg, beta[i]);
        } else {
            s[i] = 1.0f;  // fmaf(acc, 1, bias) == acc + bias exactly
            t[i] = bias ? bias[i] : 0.0f;
        }
    }
}

}  // namespace

SSAL_API int ssal_icnet_create(int c_in, int classes, ssal_icnet **out)
{
    if (!out) return fail(SSAL_EINVAL, "out is NULL");
    if (!(c_in == 1 || c_in == 3 || c_in == 4)) return fail(SSAL_EINVAL, "c_in must be 1, 3 or 4 (got %d)", c_in);
    if (classes < 2 || classes > 32) return fail(SSAL_EINVAL, "classes must be in [2,32] (got %d)", classes);
    ssal_icnet *h = new ssal_icnet();
    h->c_in = c_in;
    h->classes = classes;
    declare(h);
    *out = h;
    return SSAL_OK;
}

SSAL_API int ssal_icnet_destroy(ssal_icnet *net)
{
    if (!net) return SSAL_OK;
    if (net->arena) (void)hipFree(net->arena);
    delete net;
    return SSAL_OK;
}

SSAL_API int ssal_icnet_num_tensors(const ssal_icnet *net) { return net ? (int)net->tensors.size() : 0; }

SSAL_API int ssal_icnet_tensor_info(const ssal_icnet *net, int i, const char **name, int *ndim, int64_t dims[4])
{
    if (!net || i < 0 || i >= (int)net->tensors.size()) return fail(SSAL_EINVAL, "bad tensor index %d", i);
    const HostTensor &t = net->tensors[i];
    if (name) *name = t.name.c_str();
    if (ndim) *ndim = (int)t.dims.size();
    if (dims)
        for (size_t d = 0; d < 4; ++d) dims[d] = d < t.dims.size() ? t.dims[d] : 1;
    return SSAL_OK;
}

SSAL_API int ssal_icnet_set_tensor(ssal_icnet *net, const char *name, const float *host, int64_t numel)
{
    if (!net || !name || !host) return fail(SSAL_EINVAL, "NULL argument");
    auto it = net->index.find(name);
    if (it == net->index.end()) return fail(SSAL_EINVAL, "unknown tensor '%s'", name);
    HostTensor &t = net->tensors[it->second];
    if (numel != t.numel())
        return fail(SSAL_EINVAL, "tensor '%s': expected %lld elements, got %lld", name, (long long)t.numel(), (long long)numel);
    t.data.assign(host, host + numel);
    t.set = true;
    net->committed = false;
    return SSAL_OK;
}

SSAL_API int ssal_icnet_commit(ssal_icnet *net, void *stream)
{
    if (!net) return fail(SSAL_EINVAL, "net is NULL");
    for (const auto &t : net->tensors)
        if (!t.set) return fail(SSAL_ESTATE, "tensor '%s' has not been set", t.name.c_str());
    ArenaBuilder ab;
    struct Off { size_t w, s, t, hwio, wq, w3, pk3; };
    std::map<std::string, Off> offs;
    std::vector<float> s, t, wt;
    std::map<std::string, bool> wants_hwio;
    for (int i = 0; i < kNumBnecks; ++i)
        if (fused_bneck(kBnecks[i]))
            for (const char *suf : {"_1x1_reduce", "_3x3", "_1x1_increase"}) wants_hwio[std::string(kBnecks[i].name) + suf] = true;
    const size_t zeros_off = ab.push(std::vector<float>(128, 0.0f));
    for (const ConvSpec &sp : net->specs) {
        Off o;
        o.hwio = (size_t)-1;
        o.wq = (size_t)-1;
        o.w3 = (size_t)-1;
        o.pk3 = (size_t)-1;
        for (int i = 0; i < kNumBnecks; ++i)
            if (fused_bneck(kBnecks[i]) && sp.name == std::string(kBnecks[i].name) + "_1x1_reduce") {
                const std::string b = kBnecks[i].name;
                if (bottleneck_bf16x3_supported(kBnecks[i].cin, kBnecks[i].mid))  // the opt-in arithmetic mode (104 KB per block)
                    o.pk3 = ab.push(bf16x3::pack_layer(T(net, b + "_1x1_reduce.kernel").data(), T(net, b + "_3x3.kernel").data(),
                                                       nullptr, 9, T(net, b + "_1x1_increase.kernel").data()));
                o.wq = ab.push(bnk_quad_layout(T(net, b + "_1x1_reduce.kernel").data(), T(net, b + "_3x3.kernel").data(), nullptr, 9,
                                               T(net, b + "_1x1_increase.kernel").data()));
            }
        if (wants_hwio.count(sp.name)) o.hwio = ab.push(T(net, sp.name + ".kernel"));
        const std::vector<float> &k = T(net, sp.name + ".kernel");
        if (sp.cin % 32 == 0) {
            wt.resize(igemm_relayout_floats(sp.k, sp.k, sp.cin, sp.cout));
            igemm_relayout(k.data(), sp.k, sp.k, sp.cin, sp.cout, wt.data());
            o.w = ab.push(wt);
            // the opt-in arithmetic mode: the same kernel pre-split into bf16 triples, 1.5x the bytes, next to the fp32 layout
            o.w3 = ab.push(bf16x3::pack_igemm(k.data(), sp.k, sp.k, sp.cin, sp.cout));
        } else {
            o.w = ab.push(k);
        }
        if (sp.bn)
            fold_bn_padded(T(net, sp.name + ".mean").data(), T(net, sp.name + ".variance").data(),
                           T(net, sp.name + ".gamma").data(), T(net, sp.name + ".beta").data(), nullptr, sp.cout, s, t);
        else
            fold_bn_padded(nullptr, nullptr, nullptr, nullptr, T(net, sp.name + ".bias").data(), sp.cout, s, t);
        o.s = ab.push(s);
        o.t = ab.push(t);
        offs[sp.name] = o;
    }
    hipStream_t st = (hipStream_t)stream;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (net->arena && (net->arena_floats < ab.host.size() || net->device != dev)) {  // a handle lives on ONE device
        HIP_TRY(hipFree(net->arena));
        net->arena = nullptr;
    }
    if (!net->arena) {
        HIP_TRY(hipMalloc((void **)&net->arena, ab.host.size() * sizeof(float)));
        net->arena_floats = ab.host.size();
        net->device = dev;
    }
    HIP_TRY(hipMemcpyAsync(net->arena, ab.host.data(), ab.host.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // the staging vector dies at return
    net->convs.clear();
    for (const ConvSpec &sp : net->specs) {
        ConvDev d;
        d.spec = sp;
        const Off &o = offs.at(sp.name);
        d.w = net->arena + o.w;
        d.scale = net->arena + o.s;
        d.shift = net->arena + o.t;
        d.w_hwio = o.hwio == (size_t)-1 ? nullptr : net->arena + o.hwio;
        d.wq = o.wq == (size_t)-1 ? nullptr : net->arena + o.wq;
        d.w3 = o.w3 == (size_t)-1 ? nullptr : net->arena + o.w3;
        d.pk3 = o.pk3 == (size_t)-1 ? nullptr : net->arena + o.pk3;
        net->convs[sp.name] = d;
    }
    net->zeros128 = net->arena + zeros_off;
    net->committed = true;
    return SSAL_OK;
}

SSAL_API int64_t ssal_icnet_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    if (!net || !net->committed || n <= 0 || h <= 0 || w <= 0) return -1;
    IcWorkspace W = carve(net, nullptr, 0, n, h, w);
    return W.bytes + 256;
}

SSAL_API int ssal_icnet_forward_nhwc(ssal_icnet *net, const float *x_dev, int n, int h, int w, float *logits_dev,
                                     void *ws_dev, int64_t ws_bytes, void *stream)
{
    return forward_any(net, x_dev, false, n, h, w, logits_dev, ws_dev, ws_bytes, stream);
}

SSAL_API int ssal_icnet_forward_nhwc_u8(ssal_icnet *net, const uint8_t *x_dev, int n, int h, int w, float *logits_dev,
                                        void *ws_dev, int64_t ws_bytes, void *stream)
{
    return forward_any(net, x_dev, true, n, h, w, logits_dev, ws_dev, ws_bytes, stream);
}

SSAL_API int ssal_icnet_score_nhwc(ssal_icnet *net, const float *x_dev, int n, int h, int w, int measure,
                                   float threshold, double *scores_dev, uint8_t *label_dev, uint8_t *mask_dev,
                                   float *conf_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    return score_any(net, x_dev, false, n, h, w, measure, threshold, scores_dev, label_dev, mask_dev, conf_dev, ws_dev,
                     ws_bytes, stream);
}

SSAL_API int ssal_icnet_score_nhwc_u8(ssal_icnet *net, const uint8_t *x_dev, int n, int h, int w, int measure,
                                      float threshold, double *scores_dev, uint8_t *label_dev, uint8_t *mask_dev,
                                      float *conf_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    return score_any(net, x_dev, true, n, h, w, measure, threshold, scores_dev, label_dev, mask_dev, conf_dev, ws_dev,
                     ws_bytes, stream);
}

// ---- opt-in arithmetic (include/ssal_icnet.h): SSAL_ARITH_F32 is the plain entry ----
SSAL_API int ssal_icnet_forward_nhwc_arith(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w, int arithmetic,
                                           float *logits_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    if (arithmetic != SSAL_ARITH_F32 && arithmetic != SSAL_ARITH_BF16X3) return fail(SSAL_EINVAL, "unknown arithmetic mode %d", arithmetic);
    return forward_any(net, x_dev, x_is_u8 != 0, n, h, w, logits_dev, ws_dev, ws_bytes, stream, arithmetic);
}

SSAL_API int ssal_icnet_score_nhwc_arith(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w, int measure,
                                         float threshold, int arithmetic, double *scores_dev, uint8_t *label_dev,
                                         uint8_t *mask_dev, float *conf_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    if (arithmetic != SSAL_ARITH_F32 && arithmetic != SSAL_ARITH_BF16X3) return fail(SSAL_EINVAL, "unknown arithmetic mode %d", arithmetic);
    return score_any(net, x_dev, x_is_u8 != 0, n, h, w, measure, threshold, scores_dev, label_dev, mask_dev, conf_dev, ws_dev,
                     ws_bytes, stream, arithmetic);
}

// ---- region-level acquisition through the confidence plane (a fused tail inside k_upscore is not built: its partials
// are linear 256-pixel blocks, not tiles) ----
SSAL_API int64_t ssal_icnet_regions_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    const int64_t base = ssal_icnet_workspace_bytes(net, n, h, w);
    return base < 0 ? base : base + (int64_t)n * h * w * 4 + 256;
}

SSAL_API int ssal_icnet_score_regions_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w, int measure,
                                           float threshold, int rh, int rw, double *scores_dev, double *region_scores_dev,
                                           uint8_t *label_dev, uint8_t *mask_dev, float *conf_dev, void *ws_dev,
                                           int64_t ws_bytes, void *stream)
{
    // the region arguments are judged first: they need neither a handle nor a device
    int rc = region_check(h, w, rh, rw, false);
    if (rc) return rc;
    if (!region_scores_dev) return fail(SSAL_EINVAL, "region_scores_dev is NULL");
    if ((rc = check_dims(net, n, h, w))) return rc;
    if (!region_plane_fits(n, h, w, rh, rw))
        return fail(SSAL_EINVAL, "too many regions for one launch (n=%d h=%d w=%d rh=%d rw=%d): split the batch", n, h, w, rh, rw);
    float *plane = conf_dev;
    if (!plane && ws_dev) {  // the plane sits behind the buffers of the plain score call
        Bump b(ws_dev, ws_bytes);
        b.off = carve(net, nullptr, 0, n, h, w).bytes;
        plane = b.take<float>((int64_t)n * h * w);
        if (!b.ok) return fail(SSAL_ENOMEM, "workspace too small: need %lld bytes, got %lld",
                               (long long)ssal_icnet_regions_workspace_bytes(net, n, h, w), (long long)ws_bytes);
    }
    if ((rc = score_any(net, x_dev, x_is_u8 != 0, n, h, w, measure, threshold, scores_dev, label_dev, mask_dev, plane, ws_dev,
                        ws_bytes, stream)))
        return rc;
    HIP_TRY(launch_region_means_plane(plane, n, h, w, rh, rw, region_scores_dev, (hipStream_t)stream));
    return SSAL_OK;
}

// ---- evaluation pass (eval_any above): ssal_enet_evaluate_nhwc_arith's contract for the ICNet handle ----
SSAL_API int64_t ssal_icnet_eval_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    return eval_workspace_bytes(net, n, h, w);
}

SSAL_API int ssal_icnet_evaluate_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                      const uint8_t *labels_dev, const uint8_t *mask_dev, int64_t *confusion_dev,
                                      void *ws_dev, int64_t ws_bytes, void *stream)
{
    return eval_any(net, x_dev, x_is_u8 != 0, n, h, w, labels_dev, mask_dev, confusion_dev, ws_dev, ws_bytes, stream);
}

SSAL_API int ssal_icnet_num_endpoints(const ssal_icnet *net) { return net ? (int)net->acts.size() : 0; }

SSAL_API int ssal_icnet_endpoint_name(const ssal_icnet *net, int i, const char **name)
{
    if (!net || !name || i < 0 || i >= (int)net->acts.size()) return fail(SSAL_EINVAL, "bad endpoint index %d", i);
    *name = net->acts[i].name.c_str();
    return SSAL_OK;
}

SSAL_API int ssal_icnet_endpoint_info(const ssal_icnet *net, const char *name, int n, int h, int w, int64_t *offset,
                                      int64_t dims[4])
{
    if (!net || !name || !offset || !dims) return fail(SSAL_EINVAL, "NULL argument");
    if (n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32) return fail(SSAL_EINVAL, "bad dims n=%d h=%d w=%d", n, h, w);
    Bump b((void *)256, (int64_t)1 << 62);  // same carving as the forward pass, on a fake base
    for (const ActSpec &a : net->acts) {
        const int64_t cnt = (int64_t)n * (h / a.div) * (w / a.div) * a.c;
        const char *p = (const char *)b.take<float>(cnt);
        if (a.name == name) {
            *offset = p - (const char *)256;
            dims[0] = n; dims[1] = h / a.div; dims[2] = w / a.div; dims[3] = a.c;
            return SSAL_OK;
        }
    }
    return fail(SSAL_EINVAL, "'%s' is not a materialised ICNet tensor", name);
}

// 1: a SCORE call at h x w (with the knobs as they are now) writes the named endpoint; 0: a fused launch swallows it (its
// buffer keeps whatever an earlier call left); -1 (+ last error): unknown name / bad arguments
SSAL_API int ssal_icnet_endpoint_valid_after_score(const ssal_icnet *net, const char *name, int h, int w)
{
    if (!net || !name) { (void)fail(SSAL_EINVAL, "NULL argument"); return -1; }
    if (!net->committed) { (void)fail(SSAL_ESTATE, "ssal_icnet_commit() has not been called"); return -1; }
    if (h <= 0 || w <= 0 || h % 32 || w % 32) { (void)fail(SSAL_EINVAL, "bad dims h=%d w=%d", h, w); return -1; }
    bool known = false;
    for (const ActSpec &a : net->acts) known = known || a.name == name;
    if (!known) { (void)fail(SSAL_EINVAL, "'%s' is not a materialised ICNet tensor", name); return -1; }
    std::set<std::string> written;
    std::vector<Grp> none;
    (void)run_trunk(net, none, false, h, w, true, &written);
    return written.count(name) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// Training of ICNet's tail over a frozen trunk (include/ssal_icnet.h; DESIGN.md sections 23, 25, 28-30, 32, 37 and 38).  Four
// depths -- the output layer (head), the last fusion stage, the whole cascade head, the high-resolution branch down to the image
// -- each entered from cached features or from images, plain or semi-supervised.  Every depth is ONE description (HeadDepth,
// FusionDepth, CascadeDepth, HighresDepth), which states what differs and contains the depth above it.  What is done with a
// description is written once: depth_carve and depth_bytes (the queries and the entries' workspace check both read it), the
// body depth_run (the features, the features of the undistorted frames, an optional SemiArgs), its features wrapper
// features_entry and its images wrapper images_entry, which validate (dims, then the capped-dims check, then semi arguments and
// NULL pointers, then raw all-or-none, then the workspace size, all before any launch), carve and call it, and the two
// workspace queries features_query and images_query.  The public entries pack their arguments and call a wrapper.  The shared
// steps are ssal_train_host.h's, as for ENet.
// ------------------------------------------------------------------------------------------------
namespace {

// ---- the steps the entries share ----
// what a semi call adds behind the plain pieces (DESIGN.md sections 25 and 30): the confusion replicas, then (with_raw) the
// packed pseudo-target plane of the undistorted frames, one byte per loss pixel.  Plain: nothing.
struct SemiWs {
    unsigned long long *rep;
    uint8_t *tgt;
};

SemiWs semi_carve(Bump &b, int64_t n, int h8, int w8, int classes, bool semi, bool with_raw)
{
    SemiWs t;
    t.rep = semi ? b.take<unsigned long long>((int64_t)ssal::kConfMaxReps * ssal::conf_rep_stride(classes * classes)) : nullptr;
    t.tgt = semi && with_raw ? b.take<uint8_t>(n * (8 * (int64_t)h8) * (8 * (int64_t)w8)) : nullptr;
    return t;
}

// the launchers' form of a semi call (ssal_train_icnet.h): of the target launch, which only reads the rule ...
IcnetHeadSemi semi_of_targets(const SemiArgs &semi)
{
    return {semi.labelled, semi.measure, semi.threshold, nullptr, nullptr, nullptr, 0, nullptr};
}

// ... and of the gradient launch (tgt: the plane the target launch wrote, or NULL = targets from the training logits)
IcnetHeadSemi semi_of_grad(const SemiArgs &semi, const uint8_t *tgt, unsigned long long *rep, int reps)
{
    return {semi.labelled, semi.measure, semi.threshold, tgt, nullptr, rep, reps, (unsigned long long *)semi.pseudo_pixels};
}

// what a gradient call is given besides CallArgs: its feature maps in the depth's own order, of the training frames (f) and of
// the undistorted ones (raw: all or none), which the trunk brings about (an images entry: one after the other in the same
// endpoints) or the caller has; the packed variables and the frozen moving statistics (the head has none); the grid cap; the
// dims, h and w in the depth's unit; and, where the frame itself is the last input, its type and channel count
struct DepthIn {
    const void *f[4], *raw[4];
    const float *params, *stats;
    int max_workgroups, n, h, w, classes;
    bool x_is_u8 = false;
    int c_in = 0;
};

const float *F(const void *p) { return static_cast<const float *>(p); }

// ---- the four descriptions.  Each states: Ws and carve (the buffers of one gradient call behind `b`, in carve order; own_acts:
// the activations live here, where an images entry keeps them in the network's endpoints and bind points at those); fits and
// kNoun (its own limit and what the message calls it); kUnit (frame pixels per feature pixel and axis); kEndpoints (its feature
// inputs, in order; kFrame: then the frame); kLevel (where an images entry's frozen trunk stops); kStats (the entries take the
// frozen statistics); kImagesQueryFits (the images queries judge fits too); targets / grad (its launcher pair: the target
// launch runs the trained layers on the raw features into t's slots and leaves one byte per loss pixel, then the training
// features go through the same slots) ----

// the output layer (DESIGN.md sections 23 and 25; kernels: ssal_train_icnet.hip): sub12_sum [n,h8,w8,128]
struct HeadDepth {
    using Ws = IcnetHeadWs;
    static constexpr int kUnit = 8, kLevel = 0;
    static constexpr bool kK1 = true, kIncrease = true, kReduce = true, kBlock2 = true;
    static constexpr bool kStats = false, kFrame = false, kImagesQueryFits = false;
    static constexpr const char *kNoun = "head gradient kernel's", *kEndpoints[] = {"sub12_sum"};

    static Ws carve(Bump &b, int64_t n, int h8, int w8, int classes, bool own_acts)
    {
        Ws t;
        t.lq = own_acts ? b.take<float>(n * (2 * (int64_t)h8) * (2 * (int64_t)w8) * classes) : nullptr;
        t.wt = b.take<float>(icnet_head_ws_floats_wt());
        const int64_t G = IH_MAX_WG;  // (sized for the default grid: max_workgroups only lowers it)
        t.part = b.take<float>(G * icnet_head_floats(classes));
        t.lpart = b.take<double>(2 * G);
        return t;
    }
    static void bind(Ws &t, const IcWorkspace &W) { t.lq = W.act.at("conv6_cls"); }
    static bool fits(int n, int h8, int w8) { return icnet_head_fits(h8, w8) && (double)n * h8 * w8 <= 1099511627776.0; }
    static hipError_t targets(const DepthIn &in, const Ws &t, const IcnetHeadSemi &sa, uint8_t *tgt, hipStream_t s)
    {
        return launch_icnet_head_targets(F(in.raw[0]), in.n, in.h, in.w, in.classes, in.params, in.max_workgroups, t, sa, tgt, s);
    }
    static hipError_t grad(const DepthIn &in, const CallArgs &a, const Ws &t, const IcnetHeadSemi *sa)
    {
        return launch_icnet_head_grad(F(in.f[0]), in.n, in.h, in.w, in.classes, in.params, a.labels, a.mask, a.weight,
                                      a.label_smoothing, in.max_workgroups, t, a.loss, a.grad, a.s, sa);
    }
};

// the last fusion stage (DESIGN.md sections 28 and 30; kernels: ssal_train_icnet_fusion.hip): sub24_sum [n,h16,w16,128] and
// conv3_sub1 [n,2 h16,2 w16,64]; an images entry's block and head write conv3_sub1_proj, sub12_sum and conv6_cls
struct FusionDepth {
    using Ws = IcnetFusionWs;
    static constexpr int kUnit = 16, kLevel = 1;
    static constexpr bool kK1 = true, kIncrease = true, kReduce = true, kBlock2 = true;
    static constexpr bool kStats = true, kFrame = false, kImagesQueryFits = false;
    static constexpr const char *kNoun = "fusion gradient kernels'", *kEndpoints[] = {"sub24_sum", "conv3_sub1"};

    static Ws carve(Bump &b, int64_t n, int h16, int w16, int classes, bool own_acts)
    {
        Ws t;
        const int h8 = 2 * h16, w8 = 2 * w16;
        const int64_t act = n * h8 * (int64_t)w8 * 128;
        t.wt_a = b.take<float>(FU_GA);
        t.wt_b = b.take<float>(64 * 128);
        t.rows = b.take<float>(512);
        t.proj = own_acts ? b.take<float>(act) : nullptr;
        t.sub12 = own_acts ? b.take<float>(act) : nullptr;
        t.g = b.take<float>(act);
        t.hw = b.take<float>(n * icnet_head_tiles(h8, w8) * 36 * classes);
        t.part = b.take<float>((int64_t)FU_MAX_WG * FU_PART);  // (sized for the default grid: max_workgroups only lowers it)
        t.fold = b.take<float>(FU_PART + 64);
        t.head = HeadDepth::carve(b, n, h8, w8, classes, own_acts);
        return t;
    }
    static void bind(Ws &t, const IcWorkspace &W)
    {
        t.proj = W.act.at("conv3_sub1_proj");
        t.sub12 = W.act.at("sub12_sum");
        HeadDepth::bind(t.head, W);
    }
    static bool fits(int n, int h16, int w16) { return icnet_fusion_fits(h16, w16) && (double)n * h16 * w16 <= 274877906944.0; }
    static hipError_t targets(const DepthIn &in, const Ws &t, const IcnetHeadSemi &sa, uint8_t *tgt, hipStream_t s)
    {
        return launch_icnet_fusion_targets(F(in.raw[0]), F(in.raw[1]), in.n, in.h, in.w, in.classes, in.params, in.stats,
                                           in.max_workgroups, t, sa, tgt, s);
    }
    static hipError_t grad(const DepthIn &in, const CallArgs &a, const Ws &t, const IcnetHeadSemi *sa)
    {
        return launch_icnet_fusion_grad(F(in.f[0]), F(in.f[1]), in.n, in.h, in.w, in.classes, in.params, in.stats, a.labels, a.mask,
                                        a.weight, a.label_smoothing, in.max_workgroups, t, a.loss, a.grad, a.s, sa);
    }
};

// the whole cascade head (DESIGN.md sections 29 and 30; kernels: ssal_train_icnet_cascade.hip): conv5_4_k1 [n,h32,w32,256],
// conv3_1 [n,2 h32,2 w32,256] and conv3_sub1 [n,4 h32,4 w32,64]; an images entry's two blocks and head write the endpoints from
// conv3_1_sub2_proj on
struct CascadeDepth {
    using Ws = IcnetCascadeWs;
    static constexpr int kUnit = 32, kLevel = 2;
    static constexpr bool kK1 = true, kIncrease = true, kReduce = true, kBlock2 = true;
    static constexpr bool kStats = true, kFrame = false, kImagesQueryFits = false;
    static constexpr const char *kNoun = "cascade gradient kernels'", *kEndpoints[] = {"conv5_4_k1", "conv3_1", "conv3_sub1"};

    static Ws carve(Bump &b, int64_t n, int h32, int w32, int classes, bool own_acts)
    {
        Ws t;
        const int h16 = 2 * h32, w16 = 2 * w32;
        const int64_t act = n * h16 * (int64_t)w16 * 128;
        t.wt_c = b.take<float>(CA_GC);
        t.wt_d = b.take<float>(256 * 128);
        t.rows = b.take<float>(512);
        t.proj = own_acts ? b.take<float>(act) : nullptr;
        t.sub24 = own_acts ? b.take<float>(act) : nullptr;
        t.du = b.take<float>(4 * act);
        t.g24 = b.take<float>(act);
        t.part = b.take<float>((int64_t)CA_MAX_WG * CA_PART);  // (sized for the default grid: max_workgroups only lowers it)
        t.fold = b.take<float>(CA_PART);
        t.fusion = FusionDepth::carve(b, n, h16, w16, classes, own_acts);
        return t;
    }
    static void bind(Ws &t, const IcWorkspace &W)
    {
        t.proj = W.act.at("conv3_1_sub2_proj");
        t.sub24 = W.act.at("sub24_sum");
        FusionDepth::bind(t.fusion, W);
    }
    static bool fits(int n, int h32, int w32) { return icnet_cascade_fits(h32, w32) && FusionDepth::fits(n, 2 * h32, 2 * w32); }
    static hipError_t targets(const DepthIn &in, const Ws &t, const IcnetHeadSemi &sa, uint8_t *tgt, hipStream_t s)
    {
        return launch_icnet_cascade_targets(F(in.raw[0]), F(in.raw[1]), F(in.raw[2]), in.n, in.h, in.w, in.classes, in.params,
                                            in.stats, in.max_workgroups, t, sa, tgt, s);
    }
    static hipError_t grad(const DepthIn &in, const CallArgs &a, const Ws &t, const IcnetHeadSemi *sa)
    {
        return launch_icnet_cascade_grad(F(in.f[0]), F(in.f[1]), F(in.f[2]), in.n, in.h, in.w, in.classes, in.params, in.stats,
                                         a.labels, a.mask, a.weight, a.label_smoothing, in.max_workgroups, t, a.loss, a.grad, a.s, sa);
    }
};

// the high-resolution branch down to the image (DESIGN.md sections 32 and 37; kernels: ssal_train_icnet_highres.hip): conv5_4_k1
// [n,h32,w32,256], conv3_1 [n,2 h32,2 w32,256] and the frame x [n,32 h32,32 w32,c_in], c_in 3 or 4; the trunk of an images entry
// is the two frozen branches only, and its branch, blocks and head write conv1_sub1 / conv2_sub1 / conv3_sub1 / ...
struct HighresDepth {
    using Ws = IcnetHighresWs;
    static constexpr int kUnit = 32, kLevel = 3;
    static constexpr bool kK1 = true, kIncrease = true, kReduce = true, kBlock2 = true;
    static constexpr bool kStats = true, kFrame = true, kImagesQueryFits = true;
    static constexpr const char *kNoun = "high-resolution gradient kernels'", *kEndpoints[] = {"conv5_4_k1", "conv3_1"};

    static Ws carve(Bump &b, int64_t n, int h32, int w32, int classes, bool own_acts)
    {
        Ws t;
        const int64_t px8 = n * (4 * (int64_t)h32) * (4 * (int64_t)w32);
        t.wt2 = b.take<float>(9 * 32 * 32);
        t.wt3 = b.take<float>(9 * 32 * 64);
        t.rows = b.take<float>(256);
        t.a1 = own_acts ? b.take<float>(16 * px8 * 32) : nullptr;
        t.a2 = own_acts ? b.take<float>(4 * px8 * 32) : nullptr;
        t.f3 = own_acts ? b.take<float>(px8 * 64) : nullptr;
        t.gz3 = b.take<float>(px8 * 64);
        t.gz2 = b.take<float>(4 * px8 * 32);
        t.gz1 = b.take<float>(16 * px8 * 32);
        t.part = b.take<float>((int64_t)HR_MAX_WG * HR_PART);  // (sized for the default grid: max_workgroups only lowers it)
        t.fold = b.take<float>(HR_PART);
        t.cascade = CascadeDepth::carve(b, n, h32, w32, classes, own_acts);
        return t;
    }
    static void bind(Ws &t, const IcWorkspace &W)
    {
        t.a1 = W.act.at("conv1_sub1");
        t.a2 = W.act.at("conv2_sub1");
        t.f3 = W.act.at("conv3_sub1");
        CascadeDepth::bind(t.cascade, W);
    }
    static bool fits(int n, int h32, int w32) { return icnet_highres_fits(n, h32, w32) && CascadeDepth::fits(n, h32, w32); }
    static hipError_t targets(const DepthIn &in, const Ws &t, const IcnetHeadSemi &sa, uint8_t *tgt, hipStream_t s)
    {
        return launch_icnet_highres_targets(F(in.raw[0]), F(in.raw[1]), in.raw[2], in.x_is_u8, in.c_in, in.n, in.h, in.w,
                                            in.classes, in.params, in.stats, in.max_workgroups, t, sa, tgt, s);
    }
    static hipError_t grad(const DepthIn &in, const CallArgs &a, const Ws &t, const IcnetHeadSemi *sa)
    {
        return launch_icnet_highres_grad(F(in.f[0]), F(in.f[1]), in.f[2], in.x_is_u8, in.c_in, in.n, in.h, in.w, in.classes, in.params,
                                         in.stats, a.labels, a.mask, a.weight, a.label_smoothing, in.max_workgroups, t, a.loss, a.grad,
                                         a.s, sa);
    }
};

// the pyramid head (kernels: ssal_train_icnet_pyramid.hip): conv5_3_sum [n,h32,w32,1024], conv3_1
// [n,2 h32,2 w32,256] and conv3_sub1 [n,4 h32,4 w32,64].  A sibling of the high-resolution depth: both contain the cascade
// depth (head < fusion < cascade < {high-resolution, pyramid}).  The trunk of an images entry stops where the cascade depth's
// does, and its low-resolution schedule ends after conv5_3_sum (kK1 = false); conv5_4_k1, the two blocks and the head write the
// endpoints from conv5_4_k1 on.  The semi-supervised entries are not built yet: there is no target launch.
struct PyramidDepth {
    using Ws = IcnetPyramidWs;
    static constexpr int kUnit = 32, kLevel = 2;
    static constexpr bool kK1 = false, kIncrease = true, kReduce = true, kBlock2 = true;
    static constexpr bool kStats = true, kFrame = false, kImagesQueryFits = false;
    static constexpr const char *kNoun = "pyramid gradient kernels'", *kEndpoints[] = {"conv5_3_sum", "conv3_1", "conv3_sub1"};

    static Ws carve(Bump &b, int64_t n, int h32, int w32, int classes, bool own_acts)
    {
        Ws t;
        const int64_t act = n * h32 * (int64_t)w32 * PY_CO;
        t.wt = b.take<float>(PY_G);
        t.rows = b.take<float>(2 * PY_CO);
        t.f1 = own_acts ? b.take<float>(act) : nullptr;
        t.du = b.take<float>(4 * act);
        t.g32 = b.take<float>(act);
        t.part = b.take<float>((int64_t)PY_MAX_WG * PY_PART);  // (sized for the default grid: max_workgroups only lowers it)
        t.fold = b.take<float>(PY_PART);
        t.cascade = CascadeDepth::carve(b, n, h32, w32, classes, own_acts);
        return t;
    }
    static void bind(Ws &t, const IcWorkspace &W)
    {
        t.f1 = W.act.at("conv5_4_k1");
        CascadeDepth::bind(t.cascade, W);
    }
    static bool fits(int n, int h32, int w32) { return icnet_pyramid_fits(h32, w32) && CascadeDepth::fits(n, h32, w32); }
    static hipError_t targets(const DepthIn &, const Ws &, const IcnetHeadSemi &, uint8_t *, hipStream_t)
    {
        return hipErrorNotSupported;  // (no entry hands this depth a SemiArgs)
    }
    static hipError_t grad(const DepthIn &in, const CallArgs &a, const Ws &t, const IcnetHeadSemi *)
    {
        return launch_icnet_pyramid_grad(F(in.f[0]), F(in.f[1]), F(in.f[2]), in.n, in.h, in.w, in.classes, in.params, in.stats,
                                         a.labels, a.mask, a.weight, a.label_smoothing, in.max_workgroups, t, a.loss, a.grad, a.s);
    }
};

// through the pyramid pooling (kernels: ssal_train_icnet_pool.hip): conv5_3_3x3 [n,h32,w32,256], conv5_2
// [n,h32,w32,1024] (the identity shortcut), conv3_1 and conv3_sub1.  Contains the pyramid depth (head < fusion < cascade <
// pyramid < pooling).  The trunk of an images entry stops where the pyramid depth's does, and its low-resolution schedule ends
// inside conv5_3, behind its 3 x 3 (kIncrease = false); the increase layer, the pyramid pooling, conv5_4_k1, the two blocks and
// the head write the endpoints from conv5_3 on.  The semi-supervised entries are not built yet: there is no target launch.
struct PoolDepth {
    using Ws = IcnetPoolWs;
    static constexpr int kUnit = 32, kLevel = 2;
    static constexpr bool kK1 = false, kIncrease = false, kReduce = true, kBlock2 = true;
    static constexpr bool kStats = true, kFrame = false, kImagesQueryFits = false;
    static constexpr const char *kNoun = "pooling gradient kernels'",
                                *kEndpoints[] = {"conv5_3_3x3", "conv5_2", "conv3_1", "conv3_sub1"};

    static Ws carve(Bump &b, int64_t n, int h32, int w32, int classes, bool own_acts)
    {
        Ws t;
        const int64_t act = n * h32 * (int64_t)w32 * PO_CO;
        t.wt = b.take<float>(PO_G);
        t.rows = b.take<float>(2 * PO_CO);
        t.c53 = own_acts ? b.take<float>(act) : nullptr;
        t.sum = own_acts ? b.take<float>(act) : nullptr;
        t.pooled = own_acts ? b.take<float>(ppm_scratch_floats((int)n, h32, PO_CO)) : nullptr;
        t.dsum = b.take<float>(act);
        t.cols = b.take<float>(n * h32 * (int64_t)PO_CSLOTS * PO_CO);
        t.gb = b.take<float>(n * (int64_t)PO_SLOTS * PO_CO);
        t.g53 = b.take<float>(act);
        t.part = b.take<float>((int64_t)PY_MAX_WG * PO_PART);  // (sized for the default grid: max_workgroups only lowers it)
        t.fold = b.take<float>(PO_PART);
        t.pyramid = PyramidDepth::carve(b, n, h32, w32, classes, own_acts);
        return t;
    }
    static void bind(Ws &t, const IcWorkspace &W)
    {
        t.c53 = W.act.at("conv5_3");
        t.sum = W.act.at("conv5_3_sum");
        t.pooled = W.pooled;
        PyramidDepth::bind(t.pyramid, W);
    }
    static bool fits(int n, int h32, int w32) { return icnet_pool_fits(h32, w32) && PyramidDepth::fits(n, h32, w32); }
    static hipError_t targets(const DepthIn &, const Ws &, const IcnetHeadSemi &, uint8_t *, hipStream_t)
    {
        return hipErrorNotSupported;  // (no entry hands this depth a SemiArgs)
    }
    static hipError_t grad(const DepthIn &in, const CallArgs &a, const Ws &t, const IcnetHeadSemi *)
    {
        return launch_icnet_pool_grad(F(in.f[0]), F(in.f[1]), F(in.f[2]), F(in.f[3]), in.n, in.h, in.w, in.classes, in.params,
                                      in.stats, a.labels, a.mask, a.weight, a.label_smoothing, in.max_workgroups, t, a.loss, a.grad,
                                      a.s);
    }
};

// the last backbone bottleneck (kernels: ssal_train_icnet_bneck.hip): conv5_2 [n,h32,w32,1024] (the reduce
// layer's input and the identity shortcut), conv3_1 and conv3_sub1.  Contains the pooling depth (head < fusion < cascade <
// pyramid < pooling < bottleneck).  The trunk of an images entry stops where the pooling depth's does, and its low-resolution
// schedule ends behind conv5_2 (kReduce = false); conv5_3's three layers, the pyramid pooling, conv5_4_k1, the two blocks and
// the head write the endpoints from conv5_3_1x1_reduce on.  The semi-supervised entries are not built yet: there is no target
// launch.
struct BneckDepth {
    using Ws = IcnetBneckWs;
    static constexpr int kUnit = 32, kLevel = 2;
    static constexpr bool kK1 = false, kIncrease = false, kReduce = false, kBlock2 = true;
    static constexpr bool kStats = true, kFrame = false, kImagesQueryFits = false;
    static constexpr const char *kNoun = "bottleneck gradient kernels'", *kEndpoints[] = {"conv5_2", "conv3_1", "conv3_sub1"};

    static Ws carve(Bump &b, int64_t n, int h32, int w32, int classes, bool own_acts)
    {
        Ws t;
        const int64_t act = n * h32 * (int64_t)w32 * BK_C;
        t.wt_r = b.take<float>(BK_GR);
        t.wt_3 = b.take<float>(9 * BK_C * BK_C);
        t.rows = b.take<float>(4 * BK_C);
        t.rd = own_acts ? b.take<float>(act) : nullptr;
        t.a33 = own_acts ? b.take<float>(act) : nullptr;
        t.g3 = b.take<float>(act);
        t.gr = b.take<float>(act);
        t.part3 = b.take<float>((int64_t)BK_W3_MAX_WG * BK_PART3);  // (sized for the default grid: max_workgroups only lowers it)
        t.fold3 = b.take<float>(BK_PART3);
        t.partr = b.take<float>((int64_t)PY_MAX_WG * BK_PARTR);
        t.foldr = b.take<float>(BK_PARTR);
        t.pool = PoolDepth::carve(b, n, h32, w32, classes, own_acts);
        return t;
    }
    static void bind(Ws &t, const IcWorkspace &W)
    {
        t.rd = W.act.at("conv5_3_1x1_reduce");
        t.a33 = W.act.at("conv5_3_3x3");
        PoolDepth::bind(t.pool, W);
    }
    static bool fits(int n, int h32, int w32) { return icnet_bneck_fits(h32, w32) && PoolDepth::fits(n, h32, w32); }
    static hipError_t targets(const DepthIn &, const Ws &, const IcnetHeadSemi &, uint8_t *, hipStream_t)
    {
        return hipErrorNotSupported;  // (no entry hands this depth a SemiArgs)
    }
    static hipError_t grad(const DepthIn &in, const CallArgs &a, const Ws &t, const IcnetHeadSemi *)
    {
        return launch_icnet_bneck_grad(F(in.f[0]), F(in.f[1]), F(in.f[2]), in.n, in.h, in.w, in.classes, in.params, in.stats,
                                       a.labels, a.mask, a.weight, a.label_smoothing, in.max_workgroups, t, a.loss, a.grad, a.s);
    }
};

// through conv5_2 (kernels: ssal_train_icnet_bneck2.hip): conv5_1 [n,h32,w32,1024] (conv5_2's input and
// identity shortcut), conv3_1 and conv3_sub1.  Contains the bottleneck depth (head < fusion < cascade < pyramid < pooling <
// bottleneck < this one).  The trunk of an images entry stops where the bottleneck depth's does, and its low-resolution schedule
// ends behind conv5_1 (kBlock2 = false); conv5_2's and conv5_3's layers, the pyramid pooling, conv5_4_k1, the two blocks and the
// head write the endpoints from conv5_2_1x1_reduce on.  The semi-supervised entries are not built yet: there is no target launch.
struct Bneck2Depth {
    using Ws = IcnetBneck2Ws;
    static constexpr int kUnit = 32, kLevel = 2;
    static constexpr bool kK1 = false, kIncrease = false, kReduce = false, kBlock2 = false;
    static constexpr bool kStats = true, kFrame = false, kImagesQueryFits = false;
    static constexpr const char *kNoun = "deep bottleneck gradient kernels'", *kEndpoints[] = {"conv5_1", "conv3_1", "conv3_sub1"};

    static Ws carve(Bump &b, int64_t n, int h32, int w32, int classes, bool own_acts)
    {
        Ws t;
        const int64_t pix = n * h32 * (int64_t)w32;
        t.wt_r = b.take<float>(BK_CIN * BK_C);
        t.wt_3 = b.take<float>(9 * BK_C * BK_C);
        t.wt_i = b.take<float>(PO_CIN * PO_CO);
        t.rows = b.take<float>(B2_ROWS);
        t.rd = own_acts ? b.take<float>(pix * BK_C) : nullptr;
        t.a33 = own_acts ? b.take<float>(pix * BK_C) : nullptr;
        t.c52 = own_acts ? b.take<float>(pix * BK_CIN) : nullptr;
        t.g52 = b.take<float>(pix * BK_CIN);
        t.bneck = BneckDepth::carve(b, n, h32, w32, classes, own_acts);  // (conv5_2's backward reuses its g3, gr, partials and folds)
        return t;
    }
    static void bind(Ws &t, const IcWorkspace &W)
    {
        t.rd = W.act.at("conv5_2_1x1_reduce");
        t.a33 = W.act.at("conv5_2_3x3");
        t.c52 = W.act.at("conv5_2");
        BneckDepth::bind(t.bneck, W);
    }
    static bool fits(int n, int h32, int w32) { return BneckDepth::fits(n, h32, w32); }
    static hipError_t targets(const DepthIn &, const Ws &, const IcnetHeadSemi &, uint8_t *, hipStream_t)
    {
        return hipErrorNotSupported;  // (no entry hands this depth a SemiArgs)
    }
    static hipError_t grad(const DepthIn &in, const CallArgs &a, const Ws &t, const IcnetHeadSemi *)
    {
        return launch_icnet_bneck2_grad(F(in.f[0]), F(in.f[1]), F(in.f[2]), in.n, in.h, in.w, in.classes, in.params, in.stats,
                                        a.labels, a.mask, a.weight, a.label_smoothing, in.max_workgroups, t, a.loss, a.grad, a.s);
    }
};

// ---- what is done with a description D, once.  h, w: in D's unit ----
template <typename D>
constexpr int feature_inputs() { return (int)(sizeof(D::kEndpoints) / sizeof(D::kEndpoints[0])) + D::kFrame; }

template <typename D>
struct DepthWs {
    typename D::Ws t;
    SemiWs sw;
};

template <typename D>
DepthWs<D> depth_carve(Bump &b, int n, int h, int w, int classes, bool own_acts, bool semi, bool with_raw)
{
    DepthWs<D> c;
    c.t = D::carve(b, n, h, w, classes, own_acts);
    c.sw = semi_carve(b, n, D::kUnit / 8 * h, D::kUnit / 8 * w, classes, semi, with_raw);
    return c;
}

// front: the bytes ahead of the call's own pieces (an images entry: the forward workspace)
template <typename D>
int64_t depth_bytes(int64_t front, int n, int h, int w, int classes, bool own_acts, bool semi, bool with_raw)
{
    Bump b(nullptr, 0);
    b.off = front;
    (void)depth_carve<D>(b, n, h, w, classes, own_acts, semi, with_raw);
    return b.off + 256;
}

// (n <= 0 is capped_dims_check's first message, so the limit, which the high-resolution depth states of n too, is not asked)
template <typename D>
int depth_check(int n, int h, int w, int classes, int c_in, int max_workgroups)
{
    if (int rc = capped_dims_check(n, h, w, classes, max_workgroups, n <= 0 || D::fits(n, h, w), D::kNoun)) return rc;
    if (D::kFrame && c_in != 3 && c_in != 4)
        return fail(SSAL_EINVAL, "the high-resolution trainer takes 3 or 4 input channels (got %d)", c_in);
    return SSAL_OK;
}

template <typename D, typename Trunk>
int depth_run(Trunk trunk, const DepthIn &in, const CallArgs &a, const SemiArgs *semi, const DepthWs<D> &c)
{
    const uint8_t *tgt = nullptr;
    if (in.raw[0] && semi && semi->labelled) {  // the undistorted frames' features matter only where an image is unlabelled
        if (int rc = trunk(true)) return rc;
        HIP_TRY(D::targets(in, c.t, semi_of_targets(*semi), c.sw.tgt, a.s));
        tgt = c.sw.tgt;
    }
    if (int rc = trunk(false)) return rc;
    return with_confusion(c.sw.rep, in.classes, semi ? semi->confusion : nullptr, a.s, [&](unsigned long long *rep, int reps) -> int {
        IcnetHeadSemi sa = {};
        if (semi) sa = semi_of_grad(*semi, tgt, rep, reps);
        HIP_TRY(D::grad(in, a, c.t, semi ? &sa : nullptr));
        return SSAL_OK;
    });
}

template <typename D>
int features_entry(const DepthIn &in, const CallArgs &a, const SemiArgs *semi)
{
    constexpr int N = feature_inputs<D>();
    if (int rc = depth_check<D>(in.n, in.h, in.w, in.classes, in.c_in, in.max_workgroups)) return rc;
    int given = 0, raw = 0;
    for (int i = 0; i < N; ++i) given += in.f[i] != nullptr, raw += in.raw[i] != nullptr;
    if (int rc = args_check(given == N && in.params && (in.stats || !D::kStats), a, semi)) return rc;
    if (raw != 0 && raw != N) return fail(SSAL_EINVAL, "the raw feature pointers must be given together (%d of %d)", raw, N);
    Bump b(a.ws, a.ws_bytes);
    const DepthWs<D> c = depth_carve<D>(b, in.n, in.h, in.w, in.classes, true, semi != nullptr, raw != 0);
    if (int rc = ws_check(depth_bytes<D>(0, in.n, in.h, in.w, in.classes, true, semi != nullptr, raw != 0), b, a)) return rc;
    return depth_run<D>(no_trunk, in, a, semi, c);
}

template <typename D>
int images_entry(ssal_icnet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n, int h, int w,
                 const float *params_dev, const float *stats_dev, int max_workgroups, const CallArgs &a, const SemiArgs *semi)
{
    int rc = check_dims(net, n, h, w);
    if (rc) return rc;
    const int K = net->classes, hu = h / D::kUnit, wu = w / D::kUnit;
    const bool raw = x_raw_dev != nullptr;
    if ((rc = depth_check<D>(n, hu, wu, K, net->c_in, max_workgroups))) return rc;
    if ((rc = args_check(x_dev && params_dev && (stats_dev || !D::kStats), a, semi))) return rc;
    // the call's pieces lie behind the forward workspace (not ok when that is not)
    const IcWorkspace W = carve(net, a.ws, a.ws_bytes, n, h, w);
    Bump b(a.ws, a.ws_bytes);
    b.off = W.bytes;
    b.ok = W.ok;
    DepthWs<D> c = depth_carve<D>(b, n, hu, wu, K, false, semi != nullptr, raw);
    if ((rc = ws_check(depth_bytes<D>(W.bytes, n, hu, wu, K, false, semi != nullptr, raw), b, a))) return rc;
    D::bind(c.t, W);
    DepthIn in = {{}, {}, params_dev, stats_dev, max_workgroups, n, hu, wu, K, x_is_u8 != 0, net->c_in};
    int i = 0;
    for (const char *name : D::kEndpoints) {
        in.f[i] = W.act.at(name);
        in.raw[i++] = raw ? W.act.at(name) : nullptr;
    }
    if constexpr (D::kFrame) in.f[i] = x_dev, in.raw[i] = x_raw_dev;
    // the frozen trunk, on the undistorted (of_raw) or the training frames, through the same slots of W.  It ends in front of the
    // layers being trained: run_trunk without the head, and from level 1 / 2 / 3 on without the last fusion stage / the first
    // one / the high-resolution branch; without conv5_4_k1 where the depth trains it (kK1), and from conv5_3's increase layer on
    // where it trains that (kIncrease), from conv5_3's reduce layer on where it trains the whole bottleneck (kReduce), and from
    // conv5_2's reduce layer on where it trains that block too (kBlock2)
    hipStream_t s = a.s;
    auto trunk = [=, &W](bool of_raw) -> int {
        std::vector<Grp> one(1);
        one[0] = {W, of_raw ? x_raw_dev : x_dev, n, s};
        HIP_TRY(run_trunk(net, one, x_is_u8 != 0, h, w, true, nullptr, false, D::kLevel < 1, D::kLevel < 2, D::kLevel < 3,
                          SSAL_ARITH_F32, D::kK1, D::kIncrease, D::kReduce, D::kBlock2));
        return SSAL_OK;
    };
    return depth_run<D>(trunk, in, a, semi, c);
}

template <typename D>
int64_t features_query(int n, int h, int w, int classes, bool semi, bool with_raw)
{
    return capped_dims_ok(n, classes, D::fits(n, h, w)) ? depth_bytes<D>(0, n, h, w, classes, true, semi, with_raw) : -1;
}

template <typename D>
int64_t images_query(const ssal_icnet *net, int n, int h, int w, bool semi, bool with_raw)
{
    const int hu = h / D::kUnit, wu = w / D::kUnit;
    if (!net || !net->committed || n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32 || (D::kImagesQueryFits && !D::fits(n, hu, wu)))
        return -1;
    return depth_bytes<D>(carve(net, nullptr, 0, n, h, w).bytes, n, hu, wu, net->classes, false, semi, with_raw);
}

// ---- the trained variables back into the handle ----
// Each (tensor, host pointer, count) goes into the handle's host tensors; then the named layers are re-laid-out, folded with
// the handle's moving statistics and uploaded.
struct HostUpdate {
    const char *name;
    const float *host;
    int64_t count;
};
typedef std::vector<HostUpdate> HostUpdates;

int update_packed(ssal_icnet *net, const HostUpdates &tensors, const std::set<std::string> &layers, void *stream)
{
    if (!net->committed) return fail(SSAL_ESTATE, "ssal_icnet_commit() has not been called");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != net->device)
        return fail(SSAL_ESTATE, "the handle was committed on device %d but the current device is %d (one handle per device)",
                    net->device, dev);
    for (const HostUpdate &t : tensors) net->tensors[net->index.at(t.name)].data.assign(t.host, t.host + t.count);
    hipStream_t s = (hipStream_t)stream;
    // the staging vectors live until the synchronisation below
    std::vector<std::vector<float>> keep;
    for (const ConvSpec &sp : net->specs) {
        if (!layers.count(sp.name)) continue;
        std::vector<float> wt, sc, sh;
        if (sp.cin % 32 == 0) {
            wt.resize(igemm_relayout_floats(sp.k, sp.k, sp.cin, sp.cout));
            igemm_relayout(T(net, sp.name + ".kernel").data(), sp.k, sp.k, sp.cin, sp.cout, wt.data());
            // the pre-split copy of the opt-in arithmetic mode follows the kernel it was made from
            keep.push_back(bf16x3::pack_igemm(T(net, sp.name + ".kernel").data(), sp.k, sp.k, sp.cin, sp.cout));
            HIP_TRY(hipMemcpyAsync(const_cast<float *>(net->convs.at(sp.name).w3), keep.back().data(), keep.back().size() * 4,
                                   hipMemcpyHostToDevice, s));
        } else {
            wt = T(net, sp.name + ".kernel");  // a branch's first convolution keeps HWIO, as ssal_icnet_commit stages it
        }
        if (sp.bn)
            fold_bn_padded(T(net, sp.name + ".mean").data(), T(net, sp.name + ".variance").data(),
                           T(net, sp.name + ".gamma").data(), T(net, sp.name + ".beta").data(), nullptr, sp.cout, sc, sh);
        else
            fold_bn_padded(nullptr, nullptr, nullptr, nullptr, T(net, sp.name + ".bias").data(), sp.cout, sc, sh);
        const ConvDev &c = net->convs.at(sp.name);
        const float *dst[3] = {c.w, c.scale, c.shift};
        keep.push_back(std::move(wt));
        keep.push_back(std::move(sc));
        keep.push_back(std::move(sh));
        for (int i = 0; i < 3; ++i) {
            const std::vector<float> &src = keep[keep.size() - 3 + i];
            HIP_TRY(hipMemcpyAsync(const_cast<float *>(dst[i]), src.data(), src.size() * 4, hipMemcpyHostToDevice, s));
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    return SSAL_OK;
}

// One tensor table per depth: its own rows of the packed vector at p (ssal_train_icnet*.h), then the table of the depth above
HostUpdates then(HostUpdates own, const HostUpdates &above)
{
    own.insert(own.end(), above.begin(), above.end());
    return own;
}

HostUpdates head_tensors(const float *kernel, const float *bias, int K)
{
    return {{"conv6_cls.kernel", kernel, 128 * (int64_t)K}, {"conv6_cls.bias", bias, K}};
}

HostUpdates fusion_tensors(const float *p, int K)
{
    return then({{"conv_sub2.kernel", p + FU_KA, FU_GA},
                 {"conv_sub2.gamma", p + FU_GA, 128},
                 {"conv_sub2.beta", p + FU_BA, 128},
                 {"conv3_sub1_proj.kernel", p + FU_KB, 64 * 128},
                 {"conv3_sub1_proj.gamma", p + FU_GB, 128},
                 {"conv3_sub1_proj.beta", p + FU_BB, 128}},
                head_tensors(p + FU_HEAD, p + FU_HEAD + 128 * K, K));
}

HostUpdates cascade_tensors(const float *p, int K)
{
    return then({{"conv_sub4.kernel", p + CA_KC, CA_GC},
                 {"conv_sub4.gamma", p + CA_GC, 128},
                 {"conv_sub4.beta", p + CA_BC, 128},
                 {"conv3_1_sub2_proj.kernel", p + CA_KD, 256 * 128},
                 {"conv3_1_sub2_proj.gamma", p + CA_GD, 128},
                 {"conv3_1_sub2_proj.beta", p + CA_BD, 128}},
                fusion_tensors(p + CA_FUSION, K));
}

HostUpdates highres_tensors(const float *p, int c_in, int K)
{
    const IcnetHighresOff o = icnet_highres_offsets(c_in);
    return then({{"conv1_sub1.kernel", p + o.k1, o.g1},
                 {"conv1_sub1.gamma", p + o.g1, 32},
                 {"conv1_sub1.beta", p + o.b1, 32},
                 {"conv2_sub1.kernel", p + o.k2, 9 * 32 * 32},
                 {"conv2_sub1.gamma", p + o.g2, 32},
                 {"conv2_sub1.beta", p + o.b2, 32},
                 {"conv3_sub1.kernel", p + o.k3, 9 * 32 * 64},
                 {"conv3_sub1.gamma", p + o.g3, 64},
                 {"conv3_sub1.beta", p + o.b3, 64}},
                cascade_tensors(p + o.cascade, K));
}

HostUpdates pyramid_tensors(const float *p, int K)
{
    return then({{"conv5_4_k1.kernel", p + PY_K, PY_G}, {"conv5_4_k1.gamma", p + PY_G, PY_CO}, {"conv5_4_k1.beta", p + PY_B, PY_CO}},
                cascade_tensors(p + PY_CASCADE, K));
}

HostUpdates pool_tensors(const float *p, int K)
{
    return then({{"conv5_3_1x1_increase.kernel", p + PO_K, PO_G}, {"conv5_3_1x1_increase.gamma", p + PO_G, PO_CO},
                 {"conv5_3_1x1_increase.beta", p + PO_B, PO_CO}},
                pyramid_tensors(p + PO_PYRAMID, K));
}

HostUpdates bneck_tensors(const float *p, int K)
{
    return then({{"conv5_3_1x1_reduce.kernel", p + BK_KR, BK_GR}, {"conv5_3_1x1_reduce.gamma", p + BK_GR, BK_C},
                 {"conv5_3_1x1_reduce.beta", p + BK_BR, BK_C}, {"conv5_3_3x3.kernel", p + BK_K3, 9 * BK_C * BK_C},
                 {"conv5_3_3x3.gamma", p + BK_G3, BK_C}, {"conv5_3_3x3.beta", p + BK_B3, BK_C}},
                pool_tensors(p + BK_POOL, K));
}

HostUpdates bneck2_tensors(const float *p, int K)
{
    return then({{"conv5_2_1x1_reduce.kernel", p + B2_KR, B2_GR}, {"conv5_2_1x1_reduce.gamma", p + B2_GR, BK_C},
                 {"conv5_2_1x1_reduce.beta", p + B2_BR, BK_C}, {"conv5_2_3x3.kernel", p + B2_K3, 9 * BK_C * BK_C},
                 {"conv5_2_3x3.gamma", p + B2_G3, BK_C}, {"conv5_2_3x3.beta", p + B2_B3, BK_C},
                 {"conv5_2_1x1_increase.kernel", p + B2_KI, PO_CIN * PO_CO}, {"conv5_2_1x1_increase.gamma", p + B2_GI, PO_CO},
                 {"conv5_2_1x1_increase.beta", p + B2_BI, PO_CO}},
                bneck_tensors(p + B2_BNECK, K));
}

}  // namespace

// ---- the output layer ----
SSAL_API int64_t ssal_icnet_head_grad_workspace_bytes(int n, int h, int w, int classes)
{
    return features_query<HeadDepth>(n, h, w, classes, false, false);
}

SSAL_API int ssal_icnet_head_grad_nhwc(const float *sub12_dev, int n, int h, int w, int classes, const float *head_dev,
                                       const uint8_t *labels_dev, const float *mask_dev, float weight,
                                       float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev,
                                       void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return features_entry<HeadDepth>({{sub12_dev}, {}, head_dev, nullptr, max_workgroups, n, h, w, classes}, a, nullptr);
}

SSAL_API int64_t ssal_icnet_train_head_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    return images_query<HeadDepth>(net, n, h, w, false, false);
}

SSAL_API int ssal_icnet_train_head_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                        const uint8_t *labels_dev, const float *mask_dev, const float *head_dev,
                                        float weight, float label_smoothing, int max_workgroups, double *loss_dev,
                                        float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return images_entry<HeadDepth>(net, x_dev, nullptr, x_is_u8, n, h, w, head_dev, nullptr, max_workgroups, a, nullptr);
}

SSAL_API int64_t ssal_icnet_head_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw)
{
    return features_query<HeadDepth>(n, h, w, classes, true, with_raw != 0);
}

SSAL_API int ssal_icnet_head_grad_semi_nhwc(const float *sub12_dev, const float *sub12_raw_dev, int n, int h, int w,
                                            int classes, const float *head_dev, const uint8_t *labels_dev,
                                            const float *mask_dev, const uint8_t *labelled_dev, int measure,
                                            float threshold, float weight, float label_smoothing, int max_workgroups,
                                            double *loss_dev, float *grad_dev, int64_t *confusion_dev,
                                            int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    const SemiArgs semi = {labelled_dev, measure, threshold, confusion_dev, pseudo_pixels_dev, sub12_raw_dev != nullptr};
    return features_entry<HeadDepth>({{sub12_dev}, {sub12_raw_dev}, head_dev, nullptr, max_workgroups, n, h, w, classes}, a,
                                     &semi);
}

SSAL_API int64_t ssal_icnet_train_head_semi_workspace_bytes(const ssal_icnet *net, int n, int h, int w, int with_raw)
{
    return images_query<HeadDepth>(net, n, h, w, true, with_raw != 0);
}

SSAL_API int ssal_icnet_train_head_semi_nhwc(ssal_icnet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n,
                                             int h, int w, const uint8_t *labels_dev, const float *mask_dev,
                                             const uint8_t *labelled_dev, int measure, float threshold,
                                             const float *head_dev, float weight, float label_smoothing, int max_workgroups,
                                             double *loss_dev, float *grad_dev, int64_t *confusion_dev,
                                             int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    const SemiArgs semi = {labelled_dev, measure, threshold, confusion_dev, pseudo_pixels_dev, x_raw_dev != nullptr};
    return images_entry<HeadDepth>(net, x_dev, x_raw_dev, x_is_u8, n, h, w, head_dev, nullptr, max_workgroups, a, &semi);
}

SSAL_API int ssal_icnet_update_head(ssal_icnet *net, const float *kernel_host, const float *bias_host, void *stream)
{
    if (!net || !kernel_host || !bias_host) return fail(SSAL_EINVAL, "NULL argument");
    return update_packed(net, head_tensors(kernel_host, bias_host, net->classes), {"conv6_cls"}, stream);
}

// ---- the last fusion stage ----
SSAL_API int64_t ssal_icnet_fusion_grad_workspace_bytes(int n, int h, int w, int classes)
{
    return features_query<FusionDepth>(n, h, w, classes, false, false);
}

SSAL_API int ssal_icnet_fusion_grad_nhwc(const float *sub24_dev, const float *conv3_sub1_dev, int n, int h, int w, int classes,
                                         const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                         float weight, float label_smoothing, const float *stats_dev, int max_workgroups,
                                         double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return features_entry<FusionDepth>({{sub24_dev, conv3_sub1_dev}, {}, params_dev, stats_dev, max_workgroups, n, h, w, classes},
                                       a, nullptr);
}

SSAL_API int64_t ssal_icnet_train_fusion_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    return images_query<FusionDepth>(net, n, h, w, false, false);
}

SSAL_API int ssal_icnet_train_fusion_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                          const uint8_t *labels_dev, const float *mask_dev, const float *params_dev,
                                          float weight, float label_smoothing, const float *stats_dev, int max_workgroups,
                                          double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return images_entry<FusionDepth>(net, x_dev, nullptr, x_is_u8, n, h, w, params_dev, stats_dev, max_workgroups, a, nullptr);
}

SSAL_API int64_t ssal_icnet_fusion_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw)
{
    return features_query<FusionDepth>(n, h, w, classes, true, with_raw != 0);
}

SSAL_API int ssal_icnet_fusion_grad_semi_nhwc(const float *sub24_dev, const float *conv3_sub1_dev, const float *sub24_raw_dev,
                                              const float *conv3_sub1_raw_dev, int n, int h, int w, int classes,
                                              const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                              const uint8_t *labelled_dev, int measure, float threshold, float weight,
                                              float label_smoothing, const float *stats_dev, int max_workgroups,
                                              double *loss_dev, float *grad_dev, int64_t *confusion_dev,
                                              int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    const SemiArgs semi = {labelled_dev, measure, threshold, confusion_dev, pseudo_pixels_dev, sub24_raw_dev != nullptr};
    return features_entry<FusionDepth>({{sub24_dev, conv3_sub1_dev}, {sub24_raw_dev, conv3_sub1_raw_dev}, params_dev, stats_dev,
                                        max_workgroups, n, h, w, classes}, a, &semi);
}

SSAL_API int64_t ssal_icnet_train_fusion_semi_workspace_bytes(const ssal_icnet *net, int n, int h, int w, int with_raw)
{
    return images_query<FusionDepth>(net, n, h, w, true, with_raw != 0);
}

SSAL_API int ssal_icnet_train_fusion_semi_nhwc(ssal_icnet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n,
                                               int h, int w, const uint8_t *labels_dev, const float *mask_dev,
                                               const uint8_t *labelled_dev, int measure, float threshold,
                                               const float *params_dev, float weight, float label_smoothing,
                                               const float *stats_dev, int max_workgroups, double *loss_dev, float *grad_dev,
                                               int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev,
                                               int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    const SemiArgs semi = {labelled_dev, measure, threshold, confusion_dev, pseudo_pixels_dev, x_raw_dev != nullptr};
    return images_entry<FusionDepth>(net, x_dev, x_raw_dev, x_is_u8, n, h, w, params_dev, stats_dev, max_workgroups, a, &semi);
}

SSAL_API int ssal_icnet_update_fusion(ssal_icnet *net, const float *params_host, void *stream)
{
    if (!net || !params_host) return fail(SSAL_EINVAL, "NULL argument");
    return update_packed(net, fusion_tensors(params_host, net->classes), {"conv_sub2", "conv3_sub1_proj", "conv6_cls"}, stream);
}

// ---- the whole cascade head ----
SSAL_API int64_t ssal_icnet_cascade_grad_workspace_bytes(int n, int h, int w, int classes)
{
    return features_query<CascadeDepth>(n, h, w, classes, false, false);
}

SSAL_API int ssal_icnet_cascade_grad_nhwc(const float *conv5_4_k1_dev, const float *conv3_1_dev, const float *conv3_sub1_dev,
                                          int n, int h, int w, int classes, const float *params_dev,
                                          const uint8_t *labels_dev, const float *mask_dev, float weight,
                                          float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                          float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return features_entry<CascadeDepth>({{conv5_4_k1_dev, conv3_1_dev, conv3_sub1_dev}, {}, params_dev, stats_dev, max_workgroups,
                                         n, h, w, classes}, a, nullptr);
}

SSAL_API int64_t ssal_icnet_train_cascade_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    return images_query<CascadeDepth>(net, n, h, w, false, false);
}

SSAL_API int ssal_icnet_train_cascade_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                           const uint8_t *labels_dev, const float *mask_dev, const float *params_dev,
                                           float weight, float label_smoothing, const float *stats_dev, int max_workgroups,
                                           double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return images_entry<CascadeDepth>(net, x_dev, nullptr, x_is_u8, n, h, w, params_dev, stats_dev, max_workgroups, a, nullptr);
}

SSAL_API int64_t ssal_icnet_cascade_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw)
{
    return features_query<CascadeDepth>(n, h, w, classes, true, with_raw != 0);
}

SSAL_API int ssal_icnet_cascade_grad_semi_nhwc(const float *conv5_4_k1_dev, const float *conv3_1_dev,
                                               const float *conv3_sub1_dev, const float *conv5_4_k1_raw_dev,
                                               const float *conv3_1_raw_dev, const float *conv3_sub1_raw_dev, int n, int h,
                                               int w, int classes, const float *params_dev, const uint8_t *labels_dev,
                                               const float *mask_dev, const uint8_t *labelled_dev, int measure,
                                               float threshold, float weight, float label_smoothing, const float *stats_dev,
                                               int max_workgroups, double *loss_dev, float *grad_dev, int64_t *confusion_dev,
                                               int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    const SemiArgs semi = {labelled_dev, measure, threshold, confusion_dev, pseudo_pixels_dev, conv5_4_k1_raw_dev != nullptr};
    return features_entry<CascadeDepth>({{conv5_4_k1_dev, conv3_1_dev, conv3_sub1_dev},
                                         {conv5_4_k1_raw_dev, conv3_1_raw_dev, conv3_sub1_raw_dev}, params_dev, stats_dev,
                                         max_workgroups, n, h, w, classes}, a, &semi);
}

SSAL_API int64_t ssal_icnet_train_cascade_semi_workspace_bytes(const ssal_icnet *net, int n, int h, int w, int with_raw)
{
    return images_query<CascadeDepth>(net, n, h, w, true, with_raw != 0);
}

SSAL_API int ssal_icnet_train_cascade_semi_nhwc(ssal_icnet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n,
                                                int h, int w, const uint8_t *labels_dev, const float *mask_dev,
                                                const uint8_t *labelled_dev, int measure, float threshold,
                                                const float *params_dev, float weight, float label_smoothing,
                                                const float *stats_dev, int max_workgroups, double *loss_dev, float *grad_dev,
                                                int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev,
                                                int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    const SemiArgs semi = {labelled_dev, measure, threshold, confusion_dev, pseudo_pixels_dev, x_raw_dev != nullptr};
    return images_entry<CascadeDepth>(net, x_dev, x_raw_dev, x_is_u8, n, h, w, params_dev, stats_dev, max_workgroups, a, &semi);
}

SSAL_API int ssal_icnet_update_cascade(ssal_icnet *net, const float *params_host, void *stream)
{
    if (!net || !params_host) return fail(SSAL_EINVAL, "NULL argument");
    return update_packed(net, cascade_tensors(params_host, net->classes),
                         {"conv_sub4", "conv3_1_sub2_proj", "conv_sub2", "conv3_sub1_proj", "conv6_cls"}, stream);
}

// ---- the pyramid head: conv5_4_k1 and the whole cascade head ----
SSAL_API int64_t ssal_icnet_pyramid_grad_workspace_bytes(int n, int h, int w, int classes)
{
    return features_query<PyramidDepth>(n, h, w, classes, false, false);
}

SSAL_API int ssal_icnet_pyramid_grad_nhwc(const float *conv5_3_sum_dev, const float *conv3_1_dev, const float *conv3_sub1_dev,
                                          int n, int h, int w, int classes, const float *params_dev,
                                          const uint8_t *labels_dev, const float *mask_dev, float weight,
                                          float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                          float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return features_entry<PyramidDepth>({{conv5_3_sum_dev, conv3_1_dev, conv3_sub1_dev}, {}, params_dev, stats_dev, max_workgroups,
                                         n, h, w, classes}, a, nullptr);
}

SSAL_API int64_t ssal_icnet_train_pyramid_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    return images_query<PyramidDepth>(net, n, h, w, false, false);
}

SSAL_API int ssal_icnet_train_pyramid_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                           const uint8_t *labels_dev, const float *mask_dev, const float *params_dev,
                                           float weight, float label_smoothing, const float *stats_dev, int max_workgroups,
                                           double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return images_entry<PyramidDepth>(net, x_dev, nullptr, x_is_u8, n, h, w, params_dev, stats_dev, max_workgroups, a, nullptr);
}

SSAL_API int ssal_icnet_update_pyramid(ssal_icnet *net, const float *params_host, void *stream)
{
    if (!net || !params_host) return fail(SSAL_EINVAL, "NULL argument");
    return update_packed(net, pyramid_tensors(params_host, net->classes),
                         {"conv5_4_k1", "conv_sub4", "conv3_1_sub2_proj", "conv_sub2", "conv3_sub1_proj", "conv6_cls"}, stream);
}

// ---- through the pyramid pooling: conv5_3's increase layer and the whole pyramid head ----
SSAL_API int64_t ssal_icnet_pool_grad_workspace_bytes(int n, int h, int w, int classes)
{
    return features_query<PoolDepth>(n, h, w, classes, false, false);
}

SSAL_API int ssal_icnet_pool_grad_nhwc(const float *conv5_3_3x3_dev, const float *conv5_2_dev, const float *conv3_1_dev,
                                       const float *conv3_sub1_dev, int n, int h, int w, int classes, const float *params_dev,
                                       const uint8_t *labels_dev, const float *mask_dev, float weight, float label_smoothing,
                                       const float *stats_dev, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                                       int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return features_entry<PoolDepth>({{conv5_3_3x3_dev, conv5_2_dev, conv3_1_dev, conv3_sub1_dev}, {}, params_dev, stats_dev,
                                      max_workgroups, n, h, w, classes}, a, nullptr);
}

SSAL_API int64_t ssal_icnet_train_pool_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    return images_query<PoolDepth>(net, n, h, w, false, false);
}

SSAL_API int ssal_icnet_train_pool_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                        const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                                        float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                        float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return images_entry<PoolDepth>(net, x_dev, nullptr, x_is_u8, n, h, w, params_dev, stats_dev, max_workgroups, a, nullptr);
}

SSAL_API int ssal_icnet_update_pool(ssal_icnet *net, const float *params_host, void *stream)
{
    if (!net || !params_host) return fail(SSAL_EINVAL, "NULL argument");
    return update_packed(net, pool_tensors(params_host, net->classes),
                         {"conv5_3_1x1_increase", "conv5_4_k1", "conv_sub4", "conv3_1_sub2_proj", "conv_sub2", "conv3_sub1_proj",
                          "conv6_cls"}, stream);
}

// ---- the last backbone bottleneck: conv5_3's reduce layer and 3 x 3, and everything the pooling entries train ----
SSAL_API int64_t ssal_icnet_bneck_grad_workspace_bytes(int n, int h, int w, int classes)
{
    return features_query<BneckDepth>(n, h, w, classes, false, false);
}

SSAL_API int ssal_icnet_bneck_grad_nhwc(const float *conv5_2_dev, const float *conv3_1_dev, const float *conv3_sub1_dev, int n,
                                        int h, int w, int classes, const float *params_dev, const uint8_t *labels_dev,
                                        const float *mask_dev, float weight, float label_smoothing, const float *stats_dev,
                                        int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes,
                                        void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return features_entry<BneckDepth>({{conv5_2_dev, conv3_1_dev, conv3_sub1_dev}, {}, params_dev, stats_dev, max_workgroups, n, h,
                                       w, classes}, a, nullptr);
}

SSAL_API int64_t ssal_icnet_train_bneck_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    return images_query<BneckDepth>(net, n, h, w, false, false);
}

SSAL_API int ssal_icnet_train_bneck_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                         const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                                         float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                         float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return images_entry<BneckDepth>(net, x_dev, nullptr, x_is_u8, n, h, w, params_dev, stats_dev, max_workgroups, a, nullptr);
}

SSAL_API int ssal_icnet_update_bneck(ssal_icnet *net, const float *params_host, void *stream)
{
    if (!net || !params_host) return fail(SSAL_EINVAL, "NULL argument");
    return update_packed(net, bneck_tensors(params_host, net->classes),
                         {"conv5_3_1x1_reduce", "conv5_3_3x3", "conv5_3_1x1_increase", "conv5_4_k1", "conv_sub4", "conv3_1_sub2_proj",
                          "conv_sub2", "conv3_sub1_proj", "conv6_cls"}, stream);
}

// ---- through conv5_2: the last bottleneck but one, and everything the bottleneck entries train ----
SSAL_API int64_t ssal_icnet_bneck2_grad_workspace_bytes(int n, int h, int w, int classes)
{
    return features_query<Bneck2Depth>(n, h, w, classes, false, false);
}

SSAL_API int ssal_icnet_bneck2_grad_nhwc(const float *conv5_1_dev, const float *conv3_1_dev, const float *conv3_sub1_dev, int n,
                                         int h, int w, int classes, const float *params_dev, const uint8_t *labels_dev,
                                         const float *mask_dev, float weight, float label_smoothing, const float *stats_dev,
                                         int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes,
                                         void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return features_entry<Bneck2Depth>({{conv5_1_dev, conv3_1_dev, conv3_sub1_dev}, {}, params_dev, stats_dev, max_workgroups, n, h,
                                        w, classes}, a, nullptr);
}

SSAL_API int64_t ssal_icnet_train_bneck2_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    return images_query<Bneck2Depth>(net, n, h, w, false, false);
}

SSAL_API int ssal_icnet_train_bneck2_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                          const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                                          float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                          float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return images_entry<Bneck2Depth>(net, x_dev, nullptr, x_is_u8, n, h, w, params_dev, stats_dev, max_workgroups, a, nullptr);
}

SSAL_API int ssal_icnet_update_bneck2(ssal_icnet *net, const float *params_host, void *stream)
{
    if (!net || !params_host) return fail(SSAL_EINVAL, "NULL argument");
    return update_packed(net, bneck2_tensors(params_host, net->classes),
                         {"conv5_2_1x1_reduce", "conv5_2_3x3", "conv5_2_1x1_increase", "conv5_3_1x1_reduce", "conv5_3_3x3",
                          "conv5_3_1x1_increase", "conv5_4_k1", "conv_sub4", "conv3_1_sub2_proj", "conv_sub2", "conv3_sub1_proj",
                          "conv6_cls"}, stream);
}

// ---- the high-resolution branch down to the image ----
SSAL_API int64_t ssal_icnet_highres_grad_workspace_bytes(int n, int h, int w, int classes)
{
    return features_query<HighresDepth>(n, h, w, classes, false, false);
}

SSAL_API int ssal_icnet_highres_grad_nhwc(const float *conv5_4_k1_dev, const float *conv3_1_dev, const void *x_dev, int n, int h,
                                          int w, int classes, const float *params_dev, const uint8_t *labels_dev,
                                          const float *mask_dev, float weight, float label_smoothing, const float *stats_dev,
                                          int x_is_u8, int c_in, int max_workgroups, double *loss_dev, float *grad_dev,
                                          void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return features_entry<HighresDepth>({{conv5_4_k1_dev, conv3_1_dev, x_dev}, {}, params_dev, stats_dev, max_workgroups, n, h, w,
                                         classes, x_is_u8 != 0, c_in}, a, nullptr);
}

SSAL_API int64_t ssal_icnet_train_highres_workspace_bytes(const ssal_icnet *net, int n, int h, int w)
{
    return images_query<HighresDepth>(net, n, h, w, false, false);
}

SSAL_API int ssal_icnet_train_highres_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                           const uint8_t *labels_dev, const float *mask_dev, const float *params_dev,
                                           float weight, float label_smoothing, const float *stats_dev, int max_workgroups,
                                           double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    return images_entry<HighresDepth>(net, x_dev, nullptr, x_is_u8, n, h, w, params_dev, stats_dev, max_workgroups, a, nullptr);
}

SSAL_API int64_t ssal_icnet_highres_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw)
{
    return features_query<HighresDepth>(n, h, w, classes, true, with_raw != 0);
}

SSAL_API int ssal_icnet_highres_grad_semi_nhwc(const float *conv5_4_k1_dev, const float *conv3_1_dev, const void *x_dev,
                                               const float *conv5_4_k1_raw_dev, const float *conv3_1_raw_dev,
                                               const void *x_raw_dev, int n, int h, int w, int classes, const float *params_dev,
                                               const uint8_t *labels_dev, const float *mask_dev, const uint8_t *labelled_dev,
                                               int measure, float threshold, float weight, float label_smoothing,
                                               const float *stats_dev, int x_is_u8, int c_in, int max_workgroups,
                                               double *loss_dev, float *grad_dev, int64_t *confusion_dev,
                                               int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    const SemiArgs semi = {labelled_dev, measure, threshold, confusion_dev, pseudo_pixels_dev, conv5_4_k1_raw_dev != nullptr};
    return features_entry<HighresDepth>({{conv5_4_k1_dev, conv3_1_dev, x_dev}, {conv5_4_k1_raw_dev, conv3_1_raw_dev, x_raw_dev},
                                         params_dev, stats_dev, max_workgroups, n, h, w, classes, x_is_u8 != 0, c_in}, a, &semi);
}

SSAL_API int64_t ssal_icnet_train_highres_semi_workspace_bytes(const ssal_icnet *net, int n, int h, int w, int with_raw)
{
    return images_query<HighresDepth>(net, n, h, w, true, with_raw != 0);
}

SSAL_API int ssal_icnet_train_highres_semi_nhwc(ssal_icnet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n,
                                                int h, int w, const uint8_t *labels_dev, const float *mask_dev,
                                                const uint8_t *labelled_dev, int measure, float threshold,
                                                const float *params_dev, float weight, float label_smoothing,
                                                const float *stats_dev, int max_workgroups, double *loss_dev, float *grad_dev,
                                                int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev,
                                                int64_t ws_bytes, void *stream)
{
    const CallArgs a = {labels_dev, mask_dev, weight, label_smoothing, loss_dev, grad_dev, ws_dev, ws_bytes, (hipStream_t)stream};
    const SemiArgs semi = {labelled_dev, measure, threshold, confusion_dev, pseudo_pixels_dev, x_raw_dev != nullptr};
    return images_entry<HighresDepth>(net, x_dev, x_raw_dev, x_is_u8, n, h, w, params_dev, stats_dev, max_workgroups, a, &semi);
}

SSAL_API int ssal_icnet_update_highres(ssal_icnet *net, const float *params_host, void *stream)
{
    if (!net || !params_host) return fail(SSAL_EINVAL, "NULL argument");
    if (net->c_in != 3 && net->c_in != 4)
        return fail(SSAL_EINVAL, "the high-resolution trainer takes 3 or 4 input channels (got %d)", net->c_in);
    return update_packed(net, highres_tensors(params_host, net->c_in, net->classes),
                         {"conv1_sub1", "conv2_sub1", "conv3_sub1", "conv_sub4", "conv3_1_sub2_proj", "conv_sub2", "conv3_sub1_proj",
                          "conv6_cls"}, stream);
}

// ------------------------------------------------------------------------------------------------
// stand-alone operators
// ------------------------------------------------------------------------------------------------
namespace {

// the split kernel of the opt-in mode sits behind the buffers of the exact call (256-byte aligned), on the matrix-core path only
bool conv_bn_splits(int cin, int arithmetic) { return arithmetic == SSAL_ARITH_BF16X3 && cin % 32 == 0; }

int64_t conv_bn_bytes(int kh, int kw, int cin, int cout, int arithmetic)
{
    const int64_t wfl = cin % 32 == 0 ? (int64_t)igemm_relayout_floats(kh, kw, cin, cout) : (int64_t)kh * kw * cin * cout;
    const int64_t base = (wfl + 2 * ((cout + 31) / 32 * 32)) * 4 + 1024;
    if (!conv_bn_splits(cin, arithmetic)) return base;
    return base + (int64_t)bf16x3::igemm_units(kh, kw, cin, cout) * 16 + 256;
}

int conv_bn_act_any(const float *x_dev, int n, int h, int w, int cin, const float *kernel_host, int kh, int kw, int cout,
                    int stride, int dilation, const float *mean_host, const float *var_host, const float *gamma_host,
                    const float *beta_host, const float *bias_host, const float *res_dev, int relu, int upsample2x,
                    float *y_dev, void *ws_dev, int64_t ws_bytes, void *stream, int arithmetic)
{
    if (!x_dev || !kernel_host || !y_dev || !ws_dev) return fail(SSAL_EINVAL, "NULL pointer");
    if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || stride < 1 || dilation < 1)
        return fail(SSAL_EINVAL, "bad dims");
    const bool bn = mean_host || var_host || gamma_host || beta_host;
    if (bn && !(mean_host && var_host && gamma_host && beta_host))
        return fail(SSAL_EINVAL, "batch-norm needs all of mean / variance / gamma / beta");
    if (ws_bytes < conv_bn_bytes(kh, kw, cin, cout, arithmetic))
        return fail(SSAL_ENOMEM, "workspace too small: need %lld bytes", (long long)conv_bn_bytes(kh, kw, cin, cout, arithmetic));
    const bool first = cin % 32 != 0;
    if (first && !((cin == 1 || cin == 3 || cin == 4) && kh == 3 && kw == 3 && stride == 2 && dilation == 1 &&
                   cout == 32 && relu && !res_dev && !upsample2x))
        return fail(SSAL_EINVAL, "unsupported convolution: cin %% 32 == 0, or the 3x3 / stride-2 / 32-channel first layer "
                                 "on 1, 3 or 4 channels");
    if (!first && !igemm_supported(cin, cout, kh, kw)) return fail(SSAL_EINVAL, "unsupported kernel size %dx%d", kh, kw);
    // a shape no launcher takes is an argument error, reported before anything is staged or launched (the launchers' own
    // refusal would surface as a HIP failure); the same answer as ssal_icnet_debug_conv_dispatch
    IgemmPlan plan;
    if (first ? !conv_first_fits(n, h, w, 1)
              : igemm_plan(n, h, w, cin, kh, kw, cout, stride, dilation, res_dev != nullptr, upsample2x != 0, arithmetic, &plan) != hipSuccess)
        return fail(SSAL_EINVAL, "no kernel takes this convolution (kernel size, or a tensor beyond the 32-bit offset limits)");
    hipStream_t s = (hipStream_t)stream;
    std::vector<float> sc, sh, wt;
    fold_bn_padded(mean_host, var_host, gamma_host, beta_host, bias_host, cout, sc, sh);
    if (first) wt.assign(kernel_host, kernel_host + (size_t)kh * kw * cin * cout);
    else {
        wt.resize(igemm_relayout_floats(kh, kw, cin, cout));
        igemm_relayout(kernel_host, kh, kw, cin, cout, wt.data());
    }
    Bump b(ws_dev, ws_bytes);
    float *wd = b.take<float>((int64_t)wt.size());
    float *sd = b.take<float>((int64_t)sc.size());
    float *td = b.take<float>((int64_t)sh.size());
    HIP_TRY(hipMemcpyAsync(wd, wt.data(), wt.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(sd, sc.data(), sc.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(td, sh.data(), sh.size() * 4, hipMemcpyHostToDevice, s));
    std::vector<float> w3;
    float *w3d = nullptr;
    if (!first && conv_bn_splits(cin, arithmetic)) {
        w3 = bf16x3::pack_igemm(kernel_host, kh, kw, cin, cout);
        b.off = (b.off + 255) / 256 * 256;
        w3d = b.take<float>((int64_t)w3.size());
        HIP_TRY(hipMemcpyAsync(w3d, w3.data(), w3.size() * 4, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(s));  // the staging vectors die at return
    if (first) HIP_TRY(launch_conv_first(x_dev, false, n, h, w, cin, 1, wd, sd, td, y_dev, s));
    else
        HIP_TRY(launch_igemm(x_dev, n, h, w, cin, wd, kh, kw, cout, stride, dilation, sd, td, res_dev, relu != 0,
                             upsample2x != 0, y_dev, s, arithmetic, w3d));
    return SSAL_OK;
}

}  // namespace

SSAL_API int64_t ssal_conv_bn_workspace_bytes(int kh, int kw, int cin, int cout)
{
    if (kh <= 0 || kw <= 0 || cin <= 0 || cout <= 0) return -1;
    return conv_bn_bytes(kh, kw, cin, cout, SSAL_ARITH_F32);
}

SSAL_API int64_t ssal_conv_bn_workspace_bytes_arith(int kh, int kw, int cin, int cout, int arithmetic)
{
    if (kh <= 0 || kw <= 0 || cin <= 0 || cout <= 0) return -1;
    if (arithmetic != SSAL_ARITH_F32 && arithmetic != SSAL_ARITH_BF16X3) return -1;
    return conv_bn_bytes(kh, kw, cin, cout, arithmetic);
}

SSAL_API int ssal_conv_bn_act(const float *x_dev, int n, int h, int w, int cin, const float *kernel_host, int kh,
                              int kw, int cout, int stride, int dilation, const float *mean_host,
                              const float *var_host, const float *gamma_host, const float *beta_host,
                              const float *bias_host, const float *res_dev, int relu, int upsample2x, float *y_dev,
                              void *ws_dev, int64_t ws_bytes, void *stream)
{
    return conv_bn_act_any(x_dev, n, h, w, cin, kernel_host, kh, kw, cout, stride, dilation, mean_host, var_host, gamma_host,
                           beta_host, bias_host, res_dev, relu, upsample2x, y_dev, ws_dev, ws_bytes, stream, SSAL_ARITH_F32);
}

SSAL_API int ssal_conv_bn_act_arith(const float *x_dev, int n, int h, int w, int cin, const float *kernel_host, int kh,
                                    int kw, int cout, int stride, int dilation, const float *mean_host,
                                    const float *var_host, const float *gamma_host, const float *beta_host,
                                    const float *bias_host, const float *res_dev, int relu, int upsample2x, float *y_dev,
                                    void *ws_dev, int64_t ws_bytes, void *stream, int arithmetic)
{
    if (arithmetic != SSAL_ARITH_F32 && arithmetic != SSAL_ARITH_BF16X3) return fail(SSAL_EINVAL, "unknown arithmetic mode %d", arithmetic);
    return conv_bn_act_any(x_dev, n, h, w, cin, kernel_host, kh, kw, cout, stride, dilation, mean_host, var_host, gamma_host,
                           beta_host, bias_host, res_dev, relu, upsample2x, y_dev, ws_dev, ws_bytes, stream, arithmetic);
}

SSAL_API int ssal_icnet_debug_conv_dispatch(int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int dil, int up2,
                                            int has_res, int arithmetic, int *kernel_out, int *nt_out)
{
    if (!kernel_out || !nt_out) return fail(SSAL_EINVAL, "NULL output");
    if (arithmetic != SSAL_ARITH_F32 && arithmetic != SSAL_ARITH_BF16X3) return fail(SSAL_EINVAL, "unknown arithmetic mode %d", arithmetic);
    if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || stride < 1 || dil < 1) return fail(SSAL_EINVAL, "bad dims");
    if (cin % 32 != 0) {  // ssal_conv_bn_act's first-layer path
        if (!((cin == 1 || cin == 3 || cin == 4) && kh == 3 && kw == 3 && stride == 2 && dil == 1 && cout == 32 && !has_res && !up2))
            return fail(SSAL_EINVAL, "unsupported convolution");
        if (!conv_first_fits(n, h, w, 1))
            return fail(SSAL_EINVAL, "no kernel takes this convolution (kernel size, or a tensor beyond the 32-bit offset limits)");
        *kernel_out = SSAL_ICNET_KERNEL_CONV_FIRST;
        *nt_out = 0;
        return SSAL_OK;
    }
    IgemmPlan plan;
    if (igemm_plan(n, h, w, cin, kh, kw, cout, stride, dil, has_res != 0, up2 != 0, arithmetic, &plan) != hipSuccess)
        return fail(SSAL_EINVAL, "no kernel takes this convolution (kernel size, or a tensor beyond the 32-bit offset limits)");
    *kernel_out = plan.kernel;
    *nt_out = plan.nt;
    return SSAL_OK;
}

SSAL_API int ssal_icnet_debug_highres_raw_route(int c_in, int n, int h, int w, int *fused_out)
{
    if (!fused_out) return fail(SSAL_EINVAL, "NULL output");
    if (int rc = depth_check<HighresDepth>(n, h, w, 2, c_in, 0)) return rc;
    *fused_out = icnet_highres_raw_fused(c_in, n, h, w, ssal::knobs().ic_front, ssal::mfma_family()) ? 1 : 0;
    return SSAL_OK;
}

SSAL_API int ssal_max_pool_3x3_s2(const float *x_dev, int n, int h, int w, int c, float *y_dev, void *stream)
{
    if (!x_dev || !y_dev) return fail(SSAL_EINVAL, "NULL device pointer");
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || c % 4) return fail(SSAL_EINVAL, "bad dims n=%d h=%d w=%d c=%d (c %% 4 == 0)", n, h, w, c);
    HIP_TRY(launch_maxpool3x3_s2(x_dev, n, h, w, c, y_dev, (hipStream_t)stream));
    return SSAL_OK;
}

SSAL_API int ssal_pyramid_pooling(const float *x_dev, int n, int h, int w, int c, float *y_dev, void *ws_dev,
                                  int64_t ws_bytes, void *stream)
{
    if (!x_dev || !y_dev || !ws_dev) return fail(SSAL_EINVAL, "NULL device pointer");
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || c % 4) return fail(SSAL_EINVAL, "bad dims");
    if (ws_bytes < ppm_scratch_floats(n, h, c) * 4)
        return fail(SSAL_ENOMEM, "workspace too small: need %lld bytes", (long long)ppm_scratch_floats(n, h, c) * 4);
    HIP_TRY(launch_ppm(x_dev, n, h, w, c, (float *)ws_dev, y_dev, (hipStream_t)stream));
    return SSAL_OK;
}

SSAL_API int64_t ssal_upscore_workspace_bytes(int n, int h, int w)
{
    if (n <= 0 || h <= 0 || w <= 0) return -1;
    return (int64_t)n * upscore_blocks(h, w) * 8 + 256;
}

SSAL_API int ssal_upscore_logits_nhwc(const float *lq_dev, int n, int h, int w, int classes, int measure,
                                      float threshold, double *scores_dev, uint8_t *label_dev, uint8_t *mask_dev,
                                      float *conf_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    if (measure < 0 || measure > 2) return fail(SSAL_ENOTIMPL, "Uncertainty function not implemented (measure=%d)", measure);
    if (n <= 0 || h <= 0 || w <= 0) return fail(SSAL_EINVAL, "bad dims n=%d h=%d w=%d", n, h, w);
    if (classes < 2 || classes > 32) return fail(SSAL_EINVAL, "classes must be in [2,32] (got %d)", classes);
    if (!lq_dev || !scores_dev || !ws_dev) return fail(SSAL_EINVAL, "NULL device pointer");
    if (((uintptr_t)label_dev | (uintptr_t)mask_dev) & 3 || ((uintptr_t)conf_dev & 15))
        return fail(SSAL_EINVAL, "label_dev / mask_dev must be 4-byte aligned and conf_dev 16-byte aligned");
    if (ws_bytes < ssal_upscore_workspace_bytes(n, h, w)) return fail(SSAL_ENOMEM, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Bump b(ws_dev, ws_bytes);
    double *partial = b.take<double>((int64_t)n * upscore_blocks(h, w));
    HIP_TRY(launch_upscore(lq_dev, n, h, w, classes, measure, threshold, partial, label_dev, mask_dev, conf_dev, s));
    HIP_TRY(launch_reduce_mean(partial, n, upscore_blocks(h, w), 16.0 * (double)h * (double)w, scores_dev, s));
    return SSAL_OK;
}
