// C ABI, the forward: the launch plan of the hot path, its executors, and the batch-statistics forward (mp_forward,
// mp_forward_batch_stats).
#include "host.h"
#include "mp_wino43.h"

using namespace mp_host;

namespace {

int pick_mbw(int H, int W)
{
    long long best = -1;
    int arg = 32;
    for (int mbw : {32, 16, 8}) {
        const int tw = mbw, th = 256 / mbw;
        const long long area = (long long)((H + th - 1) / th) * th * ((W + tw - 1) / tw) * tw;
        if (best < 0 || area < best) { best = area; arg = mbw; }
    }
    return arg;
}

void prof_begin(mp_handle* h, const char* name, double flop, hipStream_t s)
{
    if (!h->prof) return;
    if (h->prof_used == h->prof_entries.size()) {
        ProfEntry e{};
        (void)hipEventCreate(&e.a); (void)hipEventCreate(&e.b);
        h->prof_entries.push_back(e);
    }
    ProfEntry& e = h->prof_entries[h->prof_used];
    e.name = name; e.flop = flop;
    (void)hipEventRecord(e.a, s);
}

void prof_end(mp_handle* h, hipStream_t s)
{
    if (!h->prof) return;
    (void)hipEventRecord(h->prof_entries[h->prof_used].b, s);
    ++h->prof_used;
}

// launcher return codes: 0 launched; 1 more work items than the 32-bit tile decode addresses; 2 a layer shape the selected
// kernel is not instantiated for (a dispatch bug: the planner only selects kernels whose *_supports() said yes)
int launch_failed(mp_handle* h, int code, const char* name, int B, int H, int W)
{
    const std::string layer = std::string("mp_forward: layer ") + name;
    if (code == 1)
        return fail(h, MP_EINVAL, layer + " has too many work items for one launch (B=" + std::to_string(B) + ", " +
                                      std::to_string(H) + "x" + std::to_string(W) + "): split the batch");
    return fail(h, MP_EINVAL, layer + ": the selected convolution kernel does not cover this layer shape (" + std::to_string(H) +
                                  "x" + std::to_string(W) + ")");
}

// ---- the launch plan: which kernel runs which convolution ----------------------------------------------------------------------
// plan_encoder() and plan_heads() make every kernel choice of a forward; plan_forward() walks the encoders once and lists the
// convolution launches in order (PlannedLaunch).  run_forward() executes that list with run_first() / run_conv() and
// mp_forward_plan() reports it (plan_record()) without launching anything, so what is reported is what runs.  The launches behind
// the list (the fused head tail or the 1x1 head layers, softmax, normalisation) are straight code in run_forward().

// the values are the codes mp_plan_launch::kernel reports
enum class Kernel {
    direct = MP_PLAN_DIRECT, wino43 = MP_PLAN_WINO43, wino43b = MP_PLAN_WINO43B,
    f16 = MP_PLAN_F16, f16_res = MP_PLAN_F16_RES, f16_res_slices = MP_PLAN_F16_RES_SLICES
};

struct ConvLaunch {
    Kernel kernel = Kernel::direct;
    bool fuse_first = false;                    // the encoder's first block is evaluated inside this launch (enc.conv2)
    int in_layout = MP_LAYOUT_NHWC, out_layout = MP_LAYOUT_NHWC;    // MP_LAYOUT_* of the input / output tensor (fp32 F(4x4,3x3) launches only)
    int ks_shift = 0;                           // split-K: the input channels run as 2^ks_shift ranges (split_ws)
    bool vin = false;                           // the input is transformed once, by a pass of its own (vin_ws)
};

// conv[0].fuse_first false: the encoder's first block is a launch of its own (enc.conv1).  H, W: each layer's input frame
struct EncoderPlan { ConvLaunch conv[7]; int H[7], W[7]; };

// one convolution launch of a forward.  The workspace buffers and the image-id lists are named, not pointed to: the plan is made
// without a workspace, and run_forward<T>() resolves the names to pointers of its element type
enum class Buf { images, P, Q, X };
enum class Ids { none, thermal, optical };
struct PlannedLaunch {
    const ConvLayer* layer = nullptr;           // nullptr: the first block of `enc` as a launch of its own (c.out_layout alone is read)
    const Encoder* enc = nullptr;               // the encoder of the layer (its first block: read when c.fuse_first); heads: nullptr
    ConvLaunch c;
    int images = 0, H = 0, W = 0;               // the launch's input
    int in_cstride = 0, in_coff = 0, out_cstride = 0, out_coff = 0;
    Buf in = Buf::images, out = Buf::P;         // a fused first block reads the images; its `in` is the buffer a launch of its own writes
    Ids ids = Ids::none;
};

// 2 encoders x (first block + 7 layers) + the heads' 3x3 launch
struct ForwardPlan { PlannedLaunch launch[17]; int n = 0; };

// the profile name of a launch (mp_profile_read, mp_plan_launch::name)
const char* launch_name(const PlannedLaunch& e) { return !e.layer ? "enc.conv1" : e.c.fuse_first ? "enc.conv1+2" : e.layer->name; }

// which F(4x4,3x3) kernel a 3x3 layer at H x W goes to: wino43 = conv_wino43.hip (two waves per SIMD; reflection padding and
// frames that are multiples of the 4x4 tile; the only one that evaluates the first block inside the launch), wino43b =
// conv_wino43b.hip (one wave per SIMD; any frame size, reflection or zero padding); direct where neither does
Kernel wino43_kind(const mp_handle* h, const ConvLayer& L, int H, int W, int in_cstride, int in_coff, int out_cstride, int out_coff)
{
    if (!(L.taps == 9 && L.u43pack && h->policy.wino43)) return Kernel::direct;
    ConvParams q{};
    q.pad_zero = h->cfg.reflection_pad ? 0 : 1; q.cin = L.cin; q.cout = L.cout; q.H = H; q.W = W;
    q.in_cstride = in_cstride; q.in_coff = in_coff; q.out_cstride = out_cstride; q.out_coff = out_coff;
    if (h->policy.wino43_gen != 2 && conv_wino43_supports(q)) return Kernel::wino43;
    if (h->policy.wino43_gen != 1 && conv_wino43b_supports(q)) return Kernel::wino43b;
    return Kernel::direct;
}

// split-K and the pre-transformed input of an fp32 launch whose kernel, fuse_first and in_layout are decided
void plan_split_vin(const mp_handle* h, const ConvLayer& L, int B, int H, int W, int fwd_batch, ConvLaunch& c)
{
    if ((c.kernel != Kernel::wino43 && c.kernel != Kernel::wino43b) || c.fuse_first) return;
    if (fwd_batch <= 2 && h->policy.splitk_max > 1) {
        // single-pair latency (the reference's shipped batchsize: 1): a launch with fewer items than half the CUs (conv7 /
        // conv8 of one 480x640 pair: 40 items of 32 units on 256 CUs) cuts the input channels into 2, 4 or 8 ranges --
        // (cin / 4) / ranges units each, even and >= 4 -- as long as the items still fit the machine once.  Only for
        // forwards of one or two images (fwd_batch: the whole forward's, not an encoder's share of it): the ranges are summed
        // in another order than one accumulator chain would, and a batched forward must not change its bits with the batch
        // size (tests: HA grouping, sharded == single-rank)
        ConvParams q{};
        q.B = B; q.H = H; q.W = W; q.nslices = L.nslices;
        const long long items = conv_wino43_items(q);
        const int units = L.cin / 4;
        int ks = 0;
        while ((items << (ks + 1)) <= h->ncu && (2 << ks) <= h->policy.splitk_max && (units >> (ks + 1)) >= 4 &&
               ((units >> (ks + 1)) & 1) == 0 && ((units >> (ks + 1)) << (ks + 1)) == units) ++ks;
        if (ks > 0 && items <= 1024) c.ks_shift = ks;
    }
    // many output slices over one input (heads: 512 couts = 8 slices): transform the input ONCE (conv_wino43.hip VIN), from 4
    // slices on -- GEMM pass 0.865 ms at 75 % of the matrix pipe + 0.106 ms for the producer against 1.03 ms with the in-kernel
    // transform per slice
    c.vin = c.kernel == Kernel::wino43 && !L.pool && c.ks_shift == 0 && !c.in_layout && L.cin % 16 == 0 && L.cin <= 256 &&
            256 % (L.cin / 2) == 0 && L.cin >= 16 && h->dbg.vin && L.nslices >= 4;
}

// which fp16 kernel a layer goes to
Kernel f16_kind(const mp_handle* h, const ConvLayer& L, int in_cstride, int in_coff, bool fuse_first)
{
    ConvParamsH q{};
    q.cin = L.cin; q.cout = L.cout; q.nslices = L.nslices; q.in_cstride = in_cstride; q.in_coff = in_coff;
    if (h->dbg.f16_res && conv_f16_res_supports(q, L.taps)) return Kernel::f16_res;
    // 64 input channels, several 64-channel output slices (enc.conv5): a slice's packed weights are 72 KiB, so the
    // LDS-resident-weights kernel runs once per slice (the input is read once per slice: cheaper than streaming the weights)
    if (h->dbg.f16_res && !fuse_first && L.taps == 9 && L.cin == 64 && L.nslices > 1 && L.cout == 64 * L.nslices)
        return Kernel::f16_res_slices;
    return Kernel::f16;
}

// the launches of one encoder over nb of the forward's fwd_batch images at H x W (tensors: NHWC, channel stride = the layer's cin / cout)
EncoderPlan plan_encoder(const mp_handle* h, const Encoder& E, int nb, int fwd_batch, int H, int W)
{
    EncoderPlan P;
    if (h->cfg.mixed_precision) {
        const ConvLayer& L0 = E.conv[0];
        // the first block inside the conv2 launch (conv_f16_res.hip F1): reflection padding, the LDS-resident-weights kernel
        P.conv[0].fuse_first = h->dbg.f16_res && h->dbg.f16_fuse1 && h->cfg.reflection_pad && !E.first_pool && L0.pool &&
                               L0.cin == 64 && L0.cout == 64 && L0.nslices == 1;
    }
    // the one walk over a forward's frame sizes: the first block's pool, then every pooled layer halves them
    for (int i = 0, hh = E.first_pool ? H / 2 : H, ww = E.first_pool ? W / 2 : W; i < E.nconv; ++i) {
        const ConvLayer& L = E.conv[i];
        ConvLaunch& c = P.conv[i];
        P.H[i] = hh; P.W[i] = ww;
        if (L.pool) { hh /= 2; ww /= 2; }       // from here on: the next layer's frame
        if (h->cfg.mixed_precision) { c.kernel = f16_kind(h, L, L.cin, 0, c.fuse_first); continue; }
        c.kernel = wino43_kind(h, L, P.H[i], P.W[i], L.cin, 0, L.cout, 0);
        if (i == 0) {
            // the first block evaluated inside the conv2 launch: by conv_wino43.hip for the pooled 64 -> 64 layer with 64 real
            // channels; the direct kernels' fused loader is a 64-channel direct convolution, and with Winograd on, the standalone
            // first block + Winograd second convolution is faster than the fused direct kernel
            const bool fuse43 = c.kernel == Kernel::wino43 && h->dbg.fuse43 && L.pool && L.cin == 64 && L.cout == 64 &&
                                h->cfg.channel_version == 0 && L.u43pack_f1;
            c.fuse_first = h->dbg.fuse_first && h->cfg.channel_version == 0 && !E.first_pool && (h->policy.direct || fuse43);
        }
        // a tensor written by conv1 or an F(4x4,3x3) layer AND read by an F(4x4,3x3) layer is channel-quad planar
        // -- when the producer's stores are few: conv1, or a POOLED F(4x4,3x3) layer.  (An un-pooled layer stores 16 pixels per
        // lane and tile; planar, a store instruction then writes 16-byte pieces 64 bytes apart instead of 64-byte runs, which
        // costs the producer more than the consumer's patch DMAs gain: conv3 1.29 vs 1.17 ms.)  The encoder output stays NHWC
        // (a planar one was measured for the head convolution: slower).
        const bool producer = i == 0 ? !E.first_pool : P.conv[i - 1].kernel != Kernel::direct && E.conv[i - 1].pool;
        c.in_layout = h->dbg.planar && c.kernel != Kernel::direct && producer ? MP_LAYOUT_PLANAR : MP_LAYOUT_NHWC;
        plan_split_vin(h, L, nb, P.H[i], P.W[i], fwd_batch, c);
        // ... and column-interleaved planar behind an UN-POOLED layer, when both ends are plain conv_wino43.hip launches (the
        // any-frame kernel, the split-K reduction and the pre-transformed-input pass read and write the other two layouts only): the
        // tile columns of an item are then consecutive 16-byte pieces, so a store instruction of the producer writes whole cache
        // lines instead of 16 half lines, and the consumer's patch rows are four runs instead of 34 pieces 256 bytes or more apart
        if (i > 0 && h->dbg.xplanar && !E.conv[i - 1].pool && P.conv[i - 1].kernel == Kernel::wino43 && P.conv[i - 1].ks_shift == 0 &&
            c.kernel == Kernel::wino43 && c.ks_shift == 0 && !c.vin)
            c.in_layout = MP_LAYOUT_XPLANAR;
        if (i > 0) P.conv[i - 1].out_layout = c.in_layout;
    }
    return P;
}

// the launch of both 3x3 head convolutions over the B images of a forward at Hc x Wc = H/8 x W/8 (input: the encoder output, NHWC)
PlannedLaunch plan_heads(const mp_handle* h, int B, int Hc, int Wc)
{
    PlannedLaunch l;
    const ConvLayer& L = h->heads3;
    // X -> P; L.cin: the encoder output channels incl. padding, 128 (64 for channel_version 2)
    l.layer = &L; l.images = B; l.H = Hc; l.W = Wc; l.in = Buf::X; l.out = Buf::P; l.in_cstride = L.cin;
    l.out_cstride = h->cfg.descriptor_head ? 2 * h->head_channels : h->head_channels;
    if (h->cfg.mixed_precision) { l.c.kernel = f16_kind(h, L, L.cin, 0, false); return l; }
    l.c.kernel = wino43_kind(h, L, Hc, Wc, L.cin, 0, l.out_cstride, 0);
    plan_split_vin(h, L, B, Hc, Wc, B, l.c);
    return l;
}

// every convolution launch of a B x H x W forward up to the heads' 3x3 one, in launch order; counts: the images of the thermal /
// only encoder and of the optical one.  An encoder ping-pongs P and Q and leaves its last layer in X (its images' share of it)
ForwardPlan plan_forward(const mp_handle* h, const int counts[2], int B, int H, int W)
{
    ForwardPlan plan;
    for (int e = 0; e < 2; ++e) {
        if (counts[e] == 0) continue;
        const Encoder& E = h->enc[e];
        const EncoderPlan ep = plan_encoder(h, E, counts[e], B, H, W);
        PlannedLaunch l;                        // first the encoder's first block
        l.enc = &E; l.images = counts[e]; l.H = H; l.W = W; l.c.out_layout = ep.conv[0].in_layout;
        l.ids = !h->cfg.multispectral ? Ids::none : e == 0 ? Ids::thermal : Ids::optical;
        if (!ep.conv[0].fuse_first) plan.launch[plan.n++] = l;
        for (int i = 0; i < E.nconv; ++i) {
            l.layer = &E.conv[i]; l.c = ep.conv[i]; l.H = ep.H[i]; l.W = ep.W[i]; l.in_cstride = l.layer->cin; l.out_cstride = l.layer->cout;
            l.in = i % 2 ? Buf::Q : Buf::P; l.out = i == E.nconv - 1 ? Buf::X : i % 2 ? Buf::P : Buf::Q;
            plan.launch[plan.n++] = l;
        }
    }
    plan.launch[plan.n++] = plan_heads(h, B, H / 8, W / 8);
    return plan;
}

// ---- executors ------------------------------------------------------------------------------------------------------------------

// the pointer-free ConvParams / ConvParamsH fields of a launch of layer L that every executor sets alike; returns the tile width
template <typename P>
int conv_geometry(const mp_handle* h, const ConvLayer& L, P& p, int in_cstride, int in_coff, int out_cstride, int out_coff, int B,
                  int H, int W)
{
    p.B = B; p.H = H; p.W = W;
    p.in_cstride = in_cstride; p.in_coff = in_coff; p.cin = L.cin;
    p.out_cstride = out_cstride; p.out_coff = out_coff; p.cout = L.cout; p.nslices = L.nslices;
    p.pad_zero = h->cfg.reflection_pad ? 0 : 1; p.bn_first = h->cfg.bn_first;
    p.ncu = h->ncu; p.xcd_shift = h->xcd_shift;
    const int mbw = L.taps == 9 ? pick_mbw(H, W) : 32, th = 256 / mbw;
    if (L.taps == 9) { p.tiles_x = (W + mbw - 1) / mbw; p.tiles_y = (H + th - 1) / th; }
    else p.total_px = (long long)B * H * W;
    return mbw;
}

// ... and of a launch of the first block (Conv1Params / Conv1ParamsH)
template <typename P, typename T>
void conv1_geometry(const mp_handle* h, P& c1, const float* images, T* out, int B, int H, int W)
{
    c1.in = images; c1.out = out; c1.B = B; c1.H = H; c1.W = W;
    c1.pad_zero = h->cfg.reflection_pad ? 0 : 1; c1.bn_first = h->cfg.bn_first;
}

// everything of a planned launch's parameters that needs no workspace: what the launchers size the launch from, so also what
// plan_record() asks them with; returns the tile width
template <typename P>
int conv_params(const mp_handle* h, const PlannedLaunch& e, P& p)
{
    if constexpr (std::is_same<P, ConvParams>::value) {
        p.relu = e.layer->relu ? 1 : 0; p.persist = h->dbg.persist;
        p.in_planar = e.c.in_layout; p.out_planar = e.c.out_layout; p.ks_shift = e.c.ks_shift;
    } else {
        p.res_groups = h->dbg.f16_res_groups;
    }
    return conv_geometry(h, *e.layer, p, e.in_cstride, e.in_coff, e.out_cstride, e.out_coff, e.images, e.H, e.W);
}

// one convolution launch as planned, either precision.  ids: the image ids of e.ids, images: the forward's input (read when
// e.c.fuse_first)
template <typename T>
int run_conv(mp_handle* h, const PlannedLaunch& e, const T* in, T* out, const int* ids, const float* images, hipStream_t s)
{
    constexpr bool f16 = std::is_same<T, _Float16>::value;
    const ConvLayer& L = *e.layer;
    const ConvLaunch& c = e.c;
    typename std::conditional<f16, ConvParamsH, ConvParams>::type p{};
    const int mbw = conv_params(h, e, p);
    p.in = in; p.out = out; p.scale = L.scale; p.shift = L.shift; p.img_list = ids;
    const FirstLayer* first = c.fuse_first ? &e.enc->first : nullptr;
    if (first) {
        p.img = images; p.w1 = f16 ? first->w_h : first->w; p.b1 = f16 ? first->bias_h : first->bias;
        p.s1 = first->scale; p.t1 = first->shift;
    }
    if constexpr (f16) {
        p.wpack = L.wpack_h; p.bias = L.bias_h;
        p.dummy = static_cast<_Float16*>(h->f16_dummy.p);
    } else {
        p.wpack = c.kernel == Kernel::direct ? L.wpack : L.u43pack; p.bias = L.bias;
        if (first && c.kernel != Kernel::direct) {      // the fused F(4x4,3x3) launch: the first block's BatchNorm is folded away (build_encoder)
            p.wpack = L.u43pack_f1; p.bias = L.bias_f1; p.w1 = first->w_f1; p.b1 = first->bias_f1; p.s1 = nullptr; p.t1 = nullptr;
        }
        if (c.ks_shift) {
            const int rc = ensure(h, h->split_ws, w43_split_bytes(conv_wino43_items(p) << c.ks_shift));
            if (rc) return rc;
            p.split_scratch = static_cast<float*>(h->split_ws.p);
        }
        if (c.vin) {
            // The pre-transformed input is an OPTIONAL workspace (2.25 x the layer's input, linear in B): without it the kernel
            // transforms per slice, bit-identically -- so an allocation failure here is not a failure of the forward
            if (ensure(h, h->vin_ws, (size_t)conv_wino43_vglobal_floats(p) * 4) == MP_OK) p.vglobal = static_cast<float*>(h->vin_ws.p);
            else { (void)hipGetLastError(); h->err.clear(); }
        }
    }
    prof_begin(h, launch_name(e), 2.0 * L.taps * L.cin * L.cout * (double)e.images * e.H * e.W +
                                      (c.fuse_first ? 2.0 * 9 * 64 * (double)e.images * e.H * e.W : 0.0), s);
    int big = 0;
    if constexpr (f16) {
        if (c.kernel == Kernel::f16_res) {
            big = launch_conv_f16_res(p, mbw, L.pool, s);
        } else if (c.kernel == Kernel::f16_res_slices) {
            for (int sl = 0; sl < L.nslices && !big; ++sl) {
                ConvParamsH q = p;
                q.wpack = p.wpack + (size_t)sl * 36 * 2 * 64 * 8;
                q.bias = p.bias + 64 * sl; q.scale = p.scale + 64 * sl; q.shift = p.shift + 64 * sl;
                q.out_coff = e.out_coff + 64 * sl; q.cout = 64; q.nslices = 1;
                big = conv_f16_res_supports(q, L.taps) ? launch_conv_f16_res(q, mbw, L.pool, s) : 2;
            }
        } else {
            big = launch_conv_f16(p, L.taps, mbw, L.pool, s);
        }
    } else {
        big = c.kernel == Kernel::wino43b ? launch_conv_wino43b(p, L.pool, s)
            : c.kernel == Kernel::wino43  ? launch_conv_wino43(p, L.pool, s, c.fuse_first)
                                          : launch_conv_mfma(p, L.taps, mbw, L.pool, c.fuse_first, s);
    }
    prof_end(h, s);
    return big ? launch_failed(h, big, L.name, e.images, e.H, e.W) : MP_OK;
}

// the first block as a launch of its own (e.layer == nullptr)
template <typename T>
void run_first(mp_handle* h, const PlannedLaunch& e, const float* images, T* out, const int* ids, hipStream_t s)
{
    constexpr bool f16 = std::is_same<T, _Float16>::value;
    const Encoder& E = *e.enc;
    typename std::conditional<f16, Conv1ParamsH, Conv1Params>::type c1{};
    conv1_geometry(h, c1, images, out, e.images, e.H, e.W);
    c1.w = f16 ? E.first.w_h : E.first.w; c1.bias = f16 ? E.first.bias_h : E.first.bias;
    c1.scale = E.first.scale; c1.shift = E.first.shift; c1.img_list = ids;
    c1.pool = E.first_pool ? 1 : 0;                          // double_convolution: false -- MaxPool2d follows the block directly
    prof_begin(h, launch_name(e), 2.0 * 9 * 64 * (double)e.images * e.H * e.W, s);
    if constexpr (f16) {
        launch_conv_first_f16(c1, s);
    } else {
        c1.channels = E.first.channels; c1.out_planar = e.c.out_layout == MP_LAYOUT_PLANAR ? 1 : 0;      // for a planar consumer
        launch_conv_first(c1, s);
    }
    prof_end(h, s);
}

// forward workspace, byte offsets of: P (B*H*W*64 elements) | Q (B*H*W*16) ping-pong activations | Lg detector logits | X encoder
// output (separate from the ping-pong buffers: with two encoders the second pass would overwrite the first pass's result) | R raw
// descriptors (fp16) | lists: image ids of the two encoders of a multispectral model
struct FwdWorkspace { size_t P, Q, Lg, X, R, lists, bytes; };
FwdWorkspace fwd_workspace(bool f16, int B, int H, int W)
{
    const size_t el = f16 ? 2 : 4, px = (size_t)B * H * W, npx = px / 64;
    FwdWorkspace w{};
    w.Q = w.P + px * 64 * el;
    w.Lg = w.Q + px * 16 * el;
    w.X = w.Lg + npx * (f16 ? 128 : 80) * el;
    w.R = w.X + npx * 128 * el;
    w.lists = w.R + (f16 ? npx * 256 * el : 0);
    w.bytes = w.lists + 2 * 1024 * 4 + 256;
    return w;
}

// the images of each encoder: multispectral models route each image by is_optical (MultiPoint.py:107-122) to enc[0] (thermal) or
// enc[1] (optical), the others run enc[0] on the whole batch.  A forward uploads ids to the 1024 ints at `lists` of its workspace
struct ImageRoute {
    int counts[2] = {0, 0};
    std::vector<int> ids;           // multispectral: [0..512) thermal image ids, [512..1024) optical ids
};

ImageRoute route_images(const mp_handle* h, const unsigned char* is_optical, int B)
{
    ImageRoute r;
    if (!h->cfg.multispectral) { r.counts[0] = B; return r; }
    r.ids.assign(1024, 0);
    for (int b = 0; b < B; ++b) {
        if (is_optical[b]) r.ids[512 + r.counts[1]++] = b;
        else r.ids[r.counts[0]++] = b;
    }
    return r;
}

// the forward, either precision (fp16: fp16 activations, fp32 softmax / descriptor normalisation), of arguments check_forward
// accepted
template <typename T>
int run_forward(mp_handle* h, const float* images, const ImageRoute& route, int B, int H, int W, float* prob, float* logits, float* desc,
                hipStream_t s)
{
    constexpr bool f16 = std::is_same<T, _Float16>::value;
    const FwdWorkspace w = fwd_workspace(f16, B, H, W);
    int rc;
    if ((rc = ensure(h, h->fwd_ws, w.bytes))) return rc;
    if (f16 && (rc = ensure(h, h->f16_dummy, 4096))) return rc;
    char* ws = static_cast<char*>(h->fwd_ws.p);
    T *P = reinterpret_cast<T*>(ws + w.P), *Q = reinterpret_cast<T*>(ws + w.Q), *X = reinterpret_cast<T*>(ws + w.X);
    T *Lg = reinterpret_cast<T*>(ws + w.Lg), *R = reinterpret_cast<T*>(ws + w.R);
    int* lists = reinterpret_cast<int*>(ws + w.lists);
    if (h->prof_used > 4000) h->prof_used = 0;      // profile ring: entries accumulate until read

    if (h->cfg.multispectral)       // pageable source: the runtime stages it before returning, so `ids` may die after this
        MP_HIP(hipMemcpyAsync(lists, route.ids.data(), 1024 * 4, hipMemcpyHostToDevice, s));
    // the planned launches: the encoders and both 3x3 head convolutions (into P)
    const ForwardPlan plan = plan_forward(h, route.counts, B, H, W);
    T* const buf[] = {nullptr, P, Q, X};                // by Buf
    const int* const ids[] = {nullptr, lists, lists + 512};     // by Ids
    for (int i = 0; i < plan.n; ++i) {
        const PlannedLaunch& e = plan.launch[i];
        if (!e.layer) run_first(h, e, images, buf[(int)e.out], ids[(int)e.ids], s);
        else if ((rc = run_conv(h, e, buf[(int)e.in], buf[(int)e.out], ids[(int)e.ids], images, s))) return rc;
    }

    // the heads' tail, not planned: it is the same for every shape, and the fused launch falls back at run time
    const int Hc = H / 8, Wc = W / 8, lstride = f16 ? 128 : 80;
    const long long npx = (long long)B * Hc * Wc;
    const int D = h->cfg.descriptor_size;
    const int hc = h->head_channels;                                 // 256 (channel_version 0) or descriptor_size
    const int headc = plan.launch[plan.n - 1].out_cstride;
    // a 1x1 head layer's launch (no part of the plan): the direct / streaming fp16 kernel on channels of P from in_coff on
    auto launch1x1 = [&](const ConvLayer& L, int in_coff, int out_cstride) {
        PlannedLaunch l;
        l.layer = &L; l.c.kernel = f16 ? Kernel::f16 : Kernel::direct; l.images = B; l.H = Hc; l.W = Wc;
        l.in_cstride = headc; l.in_coff = in_coff; l.out_cstride = out_cstride;
        return l;
    };
    if (h->dbg.head_fuse && (!f16 || prob || logits || desc)) {
        // both 1x1 convolutions + BN + softmax / shuffle + normalisation in ONE launch that reads P once (head_tail*.hip).  Not
        // instantiated for every model: then its profile entry is taken back, the separate launches below are profiled instead,
        // and a note goes to stderr once per handle
        typename std::conditional<f16, HeadTailParamsH, HeadTailParams>::type t{};
        t.x = P; t.xstride = headc; t.K = hc;
        if constexpr (f16) {
            t.wdet = h->det1.wpack_h; t.bdet = h->det1.bias_h; t.wdesc = h->desc1.wpack_h; t.bdesc = h->desc1.bias_h;
        } else {
            t.wdet = h->det1.wpack; t.bdet = h->det1.bias; t.wdesc = h->desc1.wpack; t.bdesc = h->desc1.bias;
        }
        t.sdet = h->det1.scale; t.tdet = h->det1.shift; t.sdesc = h->desc1.scale; t.tdesc = h->desc1.shift;
        t.D = D; t.npx = npx; t.B = B; t.Hc = Hc; t.Wc = Wc;
        t.prob = prob; t.logits_nchw = logits; t.desc = desc;
        t.softmax_mode = h->cfg.softmax_mode; t.normalize = h->cfg.normalize_descriptors ? 1 : 0; t.ncu = h->ncu;
        prof_begin(h, "heads.tail", 2.0 * hc * (65.0 + (desc ? D : 0)) * (double)npx, s);
        int miss;
        if constexpr (f16) miss = launch_head_tail_f16(t, s); else miss = launch_head_tail(t, s);
        prof_end(h, s);
        if (!miss) return launch_status(h);
        if (h->prof) --h->prof_used;
        if (!h->head_fallback_noted) {
            h->head_fallback_noted = true;
            fprintf(stderr, "[multipoint_hip] note: fused head tail not instantiated for %d head channels / descriptor size %d: "
                            "using the separate 1x1 convolution, softmax and normalisation launches\n", hc, D);
        }
    }
    if ((rc = run_conv(h, launch1x1(h->det1, 0, lstride), P, Lg, nullptr, nullptr, s))) return rc;
    if (prob || logits) {
        prof_begin(h, "det.softmax_shuffle", 0.0, s);
        if constexpr (f16) launch_det_post_f16(Lg, lstride, B, Hc, Wc, prob, logits, h->cfg.softmax_mode, s);
        else launch_det_post(Lg, lstride, B, Hc, Wc, prob, logits, h->cfg.softmax_mode, s);
        prof_end(h, s);
    }
    if (desc) {
        T* raw;                      // fp32: the descriptors are normalised in place
        if constexpr (f16) raw = R; else raw = desc;
        if ((rc = run_conv(h, launch1x1(h->desc1, hc, D), P, raw, nullptr, nullptr, s))) return rc;
        prof_begin(h, "desc.l2norm", 0.0, s);
        if constexpr (f16) launch_desc_l2norm_f16(R, desc, npx, D, h->cfg.normalize_descriptors ? 1 : 0, s);
        else if (h->cfg.normalize_descriptors) launch_desc_l2norm(desc, desc, npx, D, 1, s);
        prof_end(h, s);
    }
    return launch_status(h);
}

// ---- the plan as records (mp_forward_plan) ---------------------------------------------------------------------------------------

// the record of a planned launch, and for the F(4x4,3x3) kernels the item shape, item count and workgroups their launchers derive
// from run_conv()'s parameters (w43_launch_tc4, w43_launch_items, persistent_grid)
mp_plan_launch plan_record(const mp_handle* h, const PlannedLaunch& e)
{
    const ConvLaunch& c = e.c;
    mp_plan_launch r{};
    r.name = launch_name(e);
    r.kernel = e.layer ? (int)c.kernel : MP_PLAN_FIRST;
    r.images = e.images; r.H = e.H; r.W = e.W;
    r.pooled = (e.layer ? e.layer->pool : e.enc->first_pool) ? 1 : 0;
    r.ks_shift = c.ks_shift; r.vin = c.vin ? 1 : 0; r.fuse_first = c.fuse_first ? 1 : 0;
    r.in_layout = c.in_layout; r.out_layout = c.out_layout;
    if (c.kernel == Kernel::wino43 || c.kernel == Kernel::wino43b) {
        ConvParams q{}, launch;
        conv_params(h, e, q);
        unsigned grid;
        r.tc4 = w43_launch_tc4(e.H, e.W, c.fuse_first);
        if (w43_launch_shape(q, r.tc4, c.ks_shift > 0, launch, grid) == 0) { r.items = launch.nitems; r.workgroups = (int)grid; }
    }
    return r;
}

// ---- the batch-statistics forward (mp_forward_batch_stats): MultiPoint.forward in training mode, forward only -------------------
// Every BatchNorm normalises with the statistics of the batch, so no BatchNorm can be folded into a convolution: each layer is
// conv (direct kernel, identity epilogue: conv + bias [+ ReLU for conv -> ReLU -> BN models], never pooled) -> bn.stats ->
// bn.finalize -> bn.apply (affine [+ ReLU for bn_first models] [+ 2x2 max-pool]).  The direct kernels serve every layer shape, so
// the plan is the same for every model: no Winograd, no fused first block, no planar tensors, no split-K, no fused head tail.

// workspace, byte offsets of: A, Bf ping-pong activations (B*H*W*64 floats each: the largest un-pooled layer output, conv1 / conv2
// at full resolution) | X encoder output | G gathered images of one encoder (multispectral) | part stats partials | ss scale and
// shift (512 each) | lists
struct BsWorkspace { size_t A, Bf, X, G, part, ss, lists, bytes; };
BsWorkspace bs_workspace(int B, int H, int W, bool multispectral)
{
    const size_t px = (size_t)B * H * W, npx = px / 64;
    BsWorkspace w{};
    w.Bf = w.A + px * 64 * 4;
    w.X = w.Bf + px * 64 * 4;
    w.G = w.X + npx * 128 * 4;
    w.part = w.G + (multispectral ? px * 4 : 0);
    w.ss = w.part + (size_t)MP_BN_MAX_PARTS * 2 * 512 * 8;
    w.lists = w.ss + 1024 * 4;
    w.bytes = w.lists + 2 * 1024 * 4 + 256;
    return w;
}

struct BsContext {
    mp_handle* h;
    double* part;
    float *scale, *shift;
    float* stats;                   // caller's statistics array or nullptr
    hipStream_t s;
};

// statistics of x [npx][C] (C = the tensor's channels incl. padding) -> scale / shift of channels [c0, c0 + nc) for BatchNorm
// layer `layer` (real channels: its own; the rest of the range is padding)
void bs_stats(BsContext& c, const float* x, long long npx, int C)
{
    prof_begin(c.h, "bn.stats", 0.0, c.s);
    launch_bn_stats(x, npx, C, C, c.part, c.s);
    prof_end(c.h, c.s);
}

void bs_finalize(BsContext& c, const float* x, long long npx, int C, int c0, int nc, int layer)
{
    const BnLayer& L = c.h->bn_layers[layer];
    prof_begin(c.h, "bn.finalize", 0.0, c.s);
    launch_bn_finalize(c.part, npx, C, x, c0, nc, L.channels, L.gamma, L.beta, c.scale, c.shift,
                       c.stats ? c.stats + L.offset : nullptr, c.stats ? c.stats + L.offset + L.channels : nullptr, c.s);
    prof_end(c.h, c.s);
}

void bs_apply(BsContext& c, const float* x, float* y, int B, int H, int W, int C, bool relu, bool pool, const int* out_list)
{
    prof_begin(c.h, "bn.apply", 0.0, c.s);
    launch_bn_apply(x, y, B, H, W, C, c.scale, c.shift, relu, pool, out_list, c.s);
    prof_end(c.h, c.s);
}

// one convolution with the identity epilogue (direct kernel; linear: no ReLU either)
int bs_conv(mp_handle* h, const ConvLayer& L, const float* in, int in_cstride, int in_coff, float* out, int out_cstride, int B, int H,
            int W, hipStream_t s)
{
    ConvParams p{};
    const int mbw = conv_geometry(h, L, p, in_cstride, in_coff, out_cstride, 0, B, H, W);
    p.in = in; p.out = out; p.wpack = L.wpack; p.bias = L.bias; p.scale = h->bn_ident; p.shift = h->bn_ident + 512;
    p.relu = L.taps == 9 && !h->cfg.bn_first;
    p.persist = h->dbg.persist;
    prof_begin(h, L.name, 2.0 * L.taps * L.cin * L.cout * (double)B * H * W, s);
    const int big = L.taps == 9 && h->cfg.bn_first ? launch_conv_mfma_linear(p, mbw, s) : launch_conv_mfma(p, L.taps, mbw, false, false, s);
    prof_end(h, s);
    return big ? launch_failed(h, big, L.name, B, H, W) : MP_OK;
}

int run_forward_batch_stats(mp_handle* h, const float* images, const ImageRoute& route, int B, int H, int W, float* logits, float* desc,
                            float* stats, hipStream_t s)
{
    const BsWorkspace w = bs_workspace(B, H, W, h->cfg.multispectral != 0);
    int rc;
    if ((rc = ensure(h, h->bs_ws, w.bytes))) return rc;
    char* ws = static_cast<char*>(h->bs_ws.p);
    float *A = reinterpret_cast<float*>(ws + w.A), *Bf = reinterpret_cast<float*>(ws + w.Bf), *X = reinterpret_cast<float*>(ws + w.X);
    float* G = reinterpret_cast<float*>(ws + w.G);
    int* lists = reinterpret_cast<int*>(ws + w.lists);
    BsContext c{h, reinterpret_cast<double*>(ws + w.part), reinterpret_cast<float*>(ws + w.ss), reinterpret_cast<float*>(ws + w.ss) + 512,
                stats, s};
    if (h->prof_used > 4000) h->prof_used = 0;
    const bool bnf = h->cfg.bn_first != 0;

    if (h->cfg.multispectral) MP_HIP(hipMemcpyAsync(lists, route.ids.data(), 1024 * 4, hipMemcpyHostToDevice, s));
    for (int e = 0; e < 2; ++e) {
        const int nb = route.counts[e];
        if (nb == 0) continue;               // an encoder without images does not run and reports no statistics
        const Encoder& E = h->enc[e];
        const int* list = h->cfg.multispectral ? lists + 512 * e : nullptr;
        const int bn0 = e * (E.nconv + 1);   // its first BatchNorm layer
        const float* img = images;
        if (list) {                          // its images as a contiguous batch
            prof_begin(h, "bn.gather", 0.0, s);
            launch_bn_gather(images, list, nb, H, W, G, s);
            prof_end(h, s);
            img = G;
        }
        Conv1Params c1{};
        conv1_geometry(h, c1, img, A, nb, H, W);
        c1.w = E.first.w; c1.bias = E.first.bias; c1.scale = h->bn_ident; c1.shift = h->bn_ident + 512;
        c1.channels = E.first.channels;
        prof_begin(h, "enc.conv1", 2.0 * 9 * E.first.channels * (double)nb * H * W, s);
        if (bnf) launch_conv_first_linear(c1, s); else launch_conv_first(c1, s);
        prof_end(h, s);
        float* buf[2] = {A, Bf};
        int cur = 0;                         // buf[cur] holds the next layer's input
        int hh = H, ww = W;
        auto bn_layer = [&](int layer, int C, bool pool, bool last) {
            // batch statistics of buf[1 - cur] (the layer's un-pooled output), then the affine into the next input
            float* y = buf[1 - cur];
            const long long npx = (long long)nb * hh * ww;
            bs_stats(c, y, npx, C);
            bs_finalize(c, y, npx, C, 0, C, bn0 + layer);
            if (last) {
                bs_apply(c, y, X, nb, hh, ww, C, bnf, pool, list);
            } else if (pool) {
                bs_apply(c, y, buf[cur], nb, hh, ww, C, bnf, true, nullptr);
            } else {
                bs_apply(c, y, y, nb, hh, ww, C, bnf, false, nullptr);
                cur = 1 - cur;
            }
            if (pool) { hh /= 2; ww /= 2; }
        };
        cur = 1;                             // conv1 wrote buf[0] = buf[1 - cur]
        bn_layer(0, E.first.channels, E.first_pool, false);
        for (int i = 0; i < E.nconv; ++i) {
            const ConvLayer& L = E.conv[i];
            if ((rc = bs_conv(h, L, buf[cur], L.cin, 0, buf[1 - cur], L.cout, nb, hh, ww, s))) return rc;
            bn_layer(i + 1, L.cout, L.pool, i == E.nconv - 1);
        }
    }

    // heads: both 3x3 convolutions in one launch (A), the 1x1 ones into Bf (detector, row stride 80) and desc / Bf + 80 npx
    const int Hc = H / 8, Wc = W / 8, lstride = 80;
    const long long npx = (long long)B * Hc * Wc;
    const int D = h->cfg.descriptor_size, hc = h->head_channels;
    const int headc = h->cfg.descriptor_head ? 2 * hc : hc;
    const int encc = h->heads3.cin;
    const int hb = (h->cfg.multispectral ? 2 : 1) * (h->enc[0].nconv + 1);      // the heads' first BatchNorm layer
    const int fb = h->cfg.final_batchnorm ? 1 : 0;
    if ((rc = bs_conv(h, h->heads3, X, encc, 0, A, headc, B, Hc, Wc, s))) return rc;
    bs_stats(c, A, npx, headc);
    bs_finalize(c, A, npx, headc, 0, hc, hb);
    if (h->cfg.descriptor_head) bs_finalize(c, A, npx, headc, hc, hc, hb + 1 + fb);
    bs_apply(c, A, A, B, Hc, Wc, headc, bnf, false, nullptr);
    float* Lg = Bf;
    if ((rc = bs_conv(h, h->det1, A, headc, 0, Lg, lstride, B, Hc, Wc, s))) return rc;
    if (fb) {
        bs_stats(c, Lg, npx, lstride);          // channels 65..79 are not written: their statistics are discarded (padding)
        bs_finalize(c, Lg, npx, lstride, 0, lstride, hb + 1);
        bs_apply(c, Lg, Lg, B, Hc, Wc, lstride, false, false, nullptr);
    }
    prof_begin(h, "det.softmax_shuffle", 0.0, s);
    launch_det_post(Lg, lstride, B, Hc, Wc, nullptr, logits, h->cfg.softmax_mode, s);
    prof_end(h, s);
    if (h->cfg.descriptor_head) {
        // the descriptor head runs without a desc output too: its statistics are part of the forward's
        float* raw = desc ? desc : Bf + npx * lstride;
        if ((rc = bs_conv(h, h->desc1, A, headc, hc, raw, D, B, Hc, Wc, s))) return rc;
        if (fb) {
            bs_stats(c, raw, npx, D);
            bs_finalize(c, raw, npx, D, 0, D, hb + 3);
            bs_apply(c, raw, raw, B, Hc, Wc, D, false, false, nullptr);
        }
        if (desc && h->cfg.normalize_descriptors) {
            prof_begin(h, "desc.l2norm", 0.0, s);
            launch_desc_l2norm(desc, desc, npx, D, 1, s);
            prof_end(h, s);
        }
    }
    return launch_status(h);
}

// the checks of a forward's arguments, in this order, each message prefixed by the entry point `fn`.  refusal: the entry point's
// own refusal of the loaded model, or nullptr; no_logits: a logits output the entry point requires is NULL
int check_forward(mp_handle* h, const std::string& fn, const char* refusal, const float* images, const unsigned char* is_optical,
                  int B, int H, int W, bool no_logits, const float* desc)
{
    if (!h->loaded) return fail(h, MP_ESTATE, fn + ": no weights loaded (call mp_load_weights)");
    if (refusal) return fail(h, MP_EINVAL, fn + ": " + refusal);
    if (!images || B <= 0 || H <= 0 || W <= 0) return fail(h, MP_EINVAL, fn + ": bad image tensor");
    if (no_logits) return fail(h, MP_EINVAL, fn + ": logits is required");
    if ((H % 8) != 0 || (W % 8) != 0)
        return fail(h, MP_EINVAL, fn + ": H and W must be divisible by 8 (got " + std::to_string(H) + "x" + std::to_string(W) + ")");
    if (desc && !h->cfg.descriptor_head) return fail(h, MP_EINVAL, fn + ": model has no descriptor head");
    if (h->cfg.multispectral && !is_optical) return fail(h, MP_EINVAL, fn + ": multispectral model needs is_optical");
    if (h->cfg.multispectral && B > 512) return fail(h, MP_EINVAL, fn + ": multispectral B > 512 unsupported");
    return MP_OK;
}

}  // namespace

extern "C" {

int mp_forward(mp_handle* h, const float* images, const unsigned char* is_optical, int B, int H, int W,
               float* prob, float* logits, float* desc, void* stream)
{
    if (!h) return MP_EINVAL;
    int rc;
    if ((rc = check_forward(h, "mp_forward", nullptr, images, is_optical, B, H, W, false, desc))) return rc;
    const ImageRoute route = route_images(h, is_optical, B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    MP_HIP(hipSetDevice(h->device));
    return h->cfg.mixed_precision ? run_forward<_Float16>(h, images, route, B, H, W, prob, logits, desc, s)
                                  : run_forward<float>(h, images, route, B, H, W, prob, logits, desc, s);
}

int mp_forward_plan(mp_handle* h, int B, int H, int W, int n_optical, mp_plan_launch* out, int capacity, int* n)
{
    if (!h) return MP_EINVAL;
    if (!n || capacity < 0 || (capacity > 0 && !out)) return fail(h, MP_EINVAL, "mp_forward_plan: NULL argument");
    *n = 0;
    if (!h->loaded) return fail(h, MP_ESTATE, "mp_forward_plan: no weights loaded (call mp_load_weights)");
    if (B <= 0 || H <= 0 || W <= 0 || (H % 8) != 0 || (W % 8) != 0)
        return fail(h, MP_EINVAL, "mp_forward_plan: B, H and W must be positive, H and W divisible by 8");
    if (n_optical < 0 || n_optical > B) return fail(h, MP_EINVAL, "mp_forward_plan: n_optical must lie in 0..B");
    const int counts[2] = {h->cfg.multispectral ? B - n_optical : B, h->cfg.multispectral ? n_optical : 0};
    const ForwardPlan plan = plan_forward(h, counts, B, H, W);
    *n = plan.n;
    for (int i = 0; i < plan.n && i < capacity; ++i) out[i] = plan_record(h, plan.launch[i]);
    return MP_OK;
}

int mp_batch_stats_count(const mp_handle* h, int* count)
{
    if (!h || !count) return MP_EINVAL;
    if (!h->loaded) return MP_ESTATE;
    *count = (int)h->bn_layers.size();
    return MP_OK;
}

int mp_batch_stats_layer(const mp_handle* h, int i, const char** name, int* channels)
{
    if (!h || !name || !channels) return MP_EINVAL;
    if (!h->loaded) return MP_ESTATE;
    if (i < 0 || i >= (int)h->bn_layers.size()) return MP_EINVAL;
    *name = h->bn_layers[i].name.c_str();
    *channels = h->bn_layers[i].channels;
    return MP_OK;
}

int mp_forward_batch_stats(mp_handle* h, const float* images, const unsigned char* is_optical, int B, int H, int W, float* logits,
                           float* desc, float* stats, void* stream)
{
    if (!h) return MP_EINVAL;
    const char* refusal =
        h->cfg.mixed_precision ? "mixed_precision models are not supported (BatchNorm with batch statistics runs on the fp32 path only)"
        : !h->cfg.batchnorm || h->bn_layers.empty() ? "the model has no BatchNorm layers (batch statistics change nothing)"
                                                    : nullptr;
    int rc;
    if ((rc = check_forward(h, "mp_forward_batch_stats", refusal, images, is_optical, B, H, W, !logits, desc))) return rc;
    const ImageRoute route = route_images(h, is_optical, B);
    // torch.nn.functional.batch_norm(training=True) refuses a layer that sees one value per channel; the smallest layers are the
    // last encoder layers and the heads at H/8 x W/8 (an encoder's share of a multispectral batch: its own images)
    const long long cells = (long long)(H / 8) * (W / 8);
    int nmin = B;
    for (int e = 0; e < 2; ++e)
        if (route.counts[e] > 0 && route.counts[e] < nmin) nmin = route.counts[e];
    if (nmin * cells <= 1)
        return fail(h, MP_EINVAL, "Expected more than 1 value per channel when training, got input size [" + std::to_string(nmin) +
                                      ", " + std::to_string(h->bn_layers.back().channels) + ", 1, 1]");
    MP_HIP(hipSetDevice(h->device));
    return run_forward_batch_stats(h, images, route, B, H, W, logits, desc, stats, static_cast<hipStream_t>(stream));
}

}  // extern "C"
