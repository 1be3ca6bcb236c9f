// C ABI, weight loading: the state_dict parsing and the repacking of every convolution's weights into the layouts the
// kernels read (mp_load_weights).
#include "host.h"

#include <map>
#include <numeric>

using namespace mp_host;

namespace {

// v as a new device array of the loaded model; D: the element type the kernels read (fp16 weights are packed as their bits)
template <typename T, typename D>
int upload(mp_handle* h, const std::vector<T>& v, D** out)
{
    static_assert(sizeof(T) == sizeof(D), "upload: element size");
    void* d = nullptr;
    MP_HIP(hipMalloc(&d, v.size() * sizeof(T)));
    h->weights.emplace_back(d, v.size() * sizeof(T));
    MP_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = static_cast<D*>(d);
    return MP_OK;
}

void free_weights(mp_handle* h)
{
    h->weights.clear();
    h->bn_layers.clear();
    h->bn_ident = nullptr;
    h->loaded = false;
}

// IEEE binary16 <-> binary32 on the host, round-to-nearest-even (what tensor.half() does)
uint16_t f2h_bits(float f)
{
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0u));
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);          // >= 65520 rounds to inf
    if (x < 0x38800000u) {                                             // below 2^-14: fp16 subnormal
        if (x < 0x33000000u) return (uint16_t)sign;                    // below 2^-25: zero
        const int e = (int)(x >> 23);
        const uint32_t m = (x & 0x7fffffu) | 0x800000u;
        const int shift = 126 - e;
        uint32_t r = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
        if (rem > halfway || (rem == halfway && (r & 1u))) ++r;
        return (uint16_t)(sign | r);
    }
    uint32_t r = (((x >> 23) - 112u) << 10) | ((x & 0x7fffffu) >> 13);
    const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) ++r;
    return (uint16_t)(sign | r);
}

float h2f_bits(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t x;
    if (e == 0) {
        if (m == 0) { x = sign; }
        else {
            int sh = 0;
            uint32_t mm = m;
            while (!(mm & 0x400u)) { mm <<= 1; ++sh; }
            x = sign | ((uint32_t)(113 - sh) << 23) | ((mm & 0x3ffu) << 13);
        }
    } else if (e == 31) {
        x = sign | 0x7f800000u | (m << 13);
    } else {
        x = sign | ((e + 112u) << 23) | (m << 13);
    }
    float f;
    std::memcpy(&f, &x, 4);
    return f;
}

float round_half(float f) { return h2f_bits(f2h_bits(f)); }

struct TensorMap {
    std::map<std::string, const mp_tensor*> m;
    std::map<std::string, bool> used;
    const float* get(const std::string& k, long long numel, std::string& err)
    {
        auto it = m.find(k);
        if (it == m.end()) { err = "missing key in state_dict: " + k; return nullptr; }
        if (it->second->numel != numel) {
            err = "size mismatch for " + k + ": got " + std::to_string(it->second->numel) +
                  " elements, expected " + std::to_string(numel);
            return nullptr;
        }
        used[k] = true;
        return it->second->data;
    }
};

// eval-mode BatchNorm2d(eps=1e-5) as y = x*scale + shift, evaluated like ATen's CPU kernel
// (batch_norm_cpu_collect_linear_and_constant_terms): invstd = 1/sqrt(var+eps); alpha = invstd*gamma;
// beta' = beta - mean*alpha, all in fp32.
bool bn_terms(TensorMap& tm, const std::string& prefix, int c, int padded, std::vector<float>& scale,
              std::vector<float>& shift, std::string& err)
{
    const float* g = tm.get(prefix + ".weight", c, err); if (!g) return false;
    const float* b = tm.get(prefix + ".bias", c, err); if (!b) return false;
    const float* m = tm.get(prefix + ".running_mean", c, err); if (!m) return false;
    const float* v = tm.get(prefix + ".running_var", c, err); if (!v) return false;
    if (tm.m.count(prefix + ".num_batches_tracked")) tm.used[prefix + ".num_batches_tracked"] = true;
    scale.assign(padded, 1.f); shift.assign(padded, 0.f);
    for (int i = 0; i < c; ++i) {
        const float invstd = 1.0f / std::sqrt(v[i] + 1e-5f);
        const float alpha = invstd * g[i];
        scale[i] = alpha;
        shift[i] = b[i] - m[i] * alpha;
    }
    return true;
}

// output channel co of tensors with couts[0], couts[1], ... output channels concatenated along O: returns the tensor, co becomes
// the channel in it
size_t source_of(const std::vector<int>& couts, int& co)
{
    size_t t = 0;
    while (co >= couts[t]) { co -= couts[t]; ++t; }
    return t;
}

// Packed B-operand layout of the MFMA convolution kernels, in chunks of 8 E input channels, E elements per lane:
//   [slice][chunk][step = tap*4 + kgroup][nblock(2)][lane(64)][E]
//   element e of lane l = W[cout = slice*64 + nblock*32 + (l&31)][cin = chunk*8E + kgroup*2E + (l>>5)*E + e][tap]
// T float: conv_mfma_kernel, E = 4; T uint16_t: conv_f16_kernel, E = 8, the binary16 bits of W.
// srcs: list of OIHW tensors concatenated along O (the two 3x3 head convs share one launch).
// cin_real < cin: the input tensor carries zero padding channels up to a multiple of the chunk (channel_version 1 / 2): their
// weights stay zero.
template <typename T>
void pack_mfma_weights(const std::vector<const float*>& srcs, const std::vector<int>& couts, int cin, int cin_real, int taps,
                       std::vector<T>& out)
{
    constexpr bool f16 = std::is_same<T, uint16_t>::value;
    constexpr int E = f16 ? 8 : 4;
    constexpr int tail = f16 ? 5 : 2;      // steps of zero padding: the kernel's weight prefetch runs this far past the last slice
    const int cout = std::accumulate(couts.begin(), couts.end(), 0);
    const int nslices = (cout + 63) / 64, nchunks = cin / (8 * E);
    out.assign((size_t)nslices * nchunks * taps * 4 * 2 * 64 * E + tail * 2 * 64 * E, T(0));
    size_t o = 0;
    for (int s = 0; s < nslices; ++s)
        for (int c = 0; c < nchunks; ++c)
            for (int tap = 0; tap < taps; ++tap)
                for (int g = 0; g < 4; ++g)
                    for (int nb = 0; nb < 2; ++nb)
                        for (int l = 0; l < 64; ++l)
                            for (int e = 0; e < E; ++e, ++o) {
                                int co = s * 64 + nb * 32 + (l & 31);
                                const int ci = c * 8 * E + g * 2 * E + (l >> 5) * E + e;
                                if (co >= cout || ci >= cin_real) continue;
                                const float w = srcs[source_of(couts, co)][((size_t)co * cin_real + ci) * taps + tap];
                                if constexpr (f16) out[o] = f2h_bits(w);
                                else out[o] = w;
                            }
}

// Winograd F(4x4,3x3) weights for conv_wino43_kernel: U[pos = 6i+j] = (G g G^T)[i][j] for the interpolation points
// {0, +a, -a, +b, -b, inf} (a = MP_W43_A, b = MP_W43_B, mp_common.h): row of point p = [1, p, p^2] / prod_{q != p} (p - q), last
// row [0, 0, 1]; evaluated in double and rounded to fp32 ONCE.  Layout = the LDS image of a unit of 4 input channels:
//   [slice64][unit = cin/4][ch(4)][cout(64)][pos(36)]
void pack_wino43_weights(const std::vector<const float*>& srcs, const std::vector<int>& couts, int cin, int cin_real,
                         std::vector<float>& out, const float* in_scale = nullptr)
{
    const double pts[5] = {0.0, MP_W43_A, -MP_W43_A, MP_W43_B, -MP_W43_B};
    double G[6][3];
    for (int k = 0; k < 5; ++k) {
        double n = 1.0;
        for (int q = 0; q < 5; ++q)
            if (q != k) n *= pts[k] - pts[q];
        G[k][0] = 1.0 / n; G[k][1] = pts[k] / n; G[k][2] = pts[k] * pts[k] / n;
    }
    G[5][0] = 0.0; G[5][1] = 0.0; G[5][2] = 1.0;
    const int cout = std::accumulate(couts.begin(), couts.end(), 0);
    const int nslices = (cout + 63) / 64, nunits = cin / 4;
    out.assign((size_t)nslices * nunits * 4 * 64 * 36, 0.f);
    for (int s = 0; s < nslices; ++s)
        for (int u = 0; u < nunits; ++u)
            for (int ch = 0; ch < 4; ++ch)
                for (int co64 = 0; co64 < 64; ++co64) {
                    int co = s * 64 + co64;
                    const int ci = u * 4 + ch;
                    if (co >= cout || ci >= cin_real) continue;
                    const float* g = srcs[source_of(couts, co)] + ((size_t)co * cin_real + ci) * 9;
                    const double sc = in_scale ? (double)in_scale[ci] : 1.0;      // (a producer's BatchNorm scale folded into this layer)
                    double tmp[6][3];
                    for (int a = 0; a < 6; ++a)
                        for (int j = 0; j < 3; ++j) tmp[a][j] = sc * (G[a][0] * g[j] + G[a][1] * g[3 + j] + G[a][2] * g[6 + j]);
                    float* o = out.data() + ((((size_t)s * nunits + u) * 4 + ch) * 64 + co64) * 36;
                    for (int a = 0; a < 6; ++a)
                        for (int b = 0; b < 6; ++b) o[6 * a + b] = (float)(tmp[a][0] * G[b][0] + tmp[a][1] * G[b][1] + tmp[a][2] * G[b][2]);
                }
}

// cin: channel count of the (zero-padded) input tensor, a multiple of 32; cin_real: channels of the reference conv.
// L.cout is rounded up to a multiple of 32: the extra output channels have zero weights/bias and identity BN, so
// the kernel writes zeros there -- exactly the padding the next layer expects.
int build_conv(mp_handle* h, TensorMap& tm, ConvLayer& L, const char* name,
               const std::vector<std::string>& conv_keys, const std::vector<std::string>& bn_keys,
               const std::vector<int>& couts, int cin, int taps, bool pool, bool relu, int cin_real = 0,
               bool pad_cout = false)
{
    if (cin_real <= 0) cin_real = cin;
    std::string err;
    const int cout = std::accumulate(couts.begin(), couts.end(), 0);
    const int padded = ((cout + 63) / 64) * 64;
    std::vector<const float*> srcs;
    std::vector<float> bias(padded, 0.f), scale(padded, 1.f), shift(padded, 0.f);
    int off = 0;
    for (size_t i = 0; i < conv_keys.size(); ++i) {
        const float* w = tm.get(conv_keys[i] + ".weight", (long long)couts[i] * cin_real * taps, err);
        if (!w) return fail(h, MP_EINVAL, err);
        const float* b = tm.get(conv_keys[i] + ".bias", couts[i], err);
        if (!b) return fail(h, MP_EINVAL, err);
        srcs.push_back(w);
        for (int c = 0; c < couts[i]; ++c) bias[off + c] = b[c];
        if (!bn_keys[i].empty()) {
            std::vector<float> s, t;
            if (!bn_terms(tm, bn_keys[i], couts[i], couts[i], s, t, err)) return fail(h, MP_EINVAL, err);
            for (int c = 0; c < couts[i]; ++c) { scale[off + c] = s[c]; shift[off + c] = t[c]; }
        }
        off += couts[i];
    }
    std::vector<float> packed;
    pack_mfma_weights(srcs, couts, cin, cin_real, taps, packed);
    const int pm = h->cfg.mixed_precision ? 64 : 32;           // channel padding granule: the fp16 kernels walk K in chunks of 64
    L.name = name; L.cin = cin; L.cout = pad_cout ? ((cout + pm - 1) / pm) * pm : cout; L.taps = taps; L.nslices = padded / 64;
    L.pool = pool; L.relu = relu;
    int rc;
    if ((rc = upload(h, packed, &L.wpack))) return rc;
    if ((rc = upload(h, bias, &L.bias))) return rc;
    if ((rc = upload(h, scale, &L.scale))) return rc;
    if ((rc = upload(h, shift, &L.shift))) return rc;
    if (taps == 9 && h->policy.wino43 && cin % 8 == 0) {
        std::vector<float> u4;
        pack_wino43_weights(srcs, couts, cin, cin_real, u4);
        if ((rc = upload(h, u4, &L.u43pack))) return rc;
    }
    if (h->cfg.mixed_precision) {
        std::vector<uint16_t> ph;
        pack_mfma_weights(srcs, couts, cin, cin_real, taps, ph);
        if ((rc = upload(h, ph, &L.wpack_h))) return rc;
        std::vector<float> bh(bias);
        for (float& v : bh) v = round_half(v);
        if ((rc = upload(h, bh, &L.bias_h))) return rc;
    }
    return MP_OK;
}

// the batch-statistics forward's record of BatchNorm layer `prefix` (appended: call in state_dict order)
int add_bn_layer(mp_handle* h, TensorMap& tm, const std::string& prefix, int channels)
{
    std::string err;
    const float* g = tm.get(prefix + ".weight", channels, err); if (!g) return fail(h, MP_EINVAL, err);
    const float* b = tm.get(prefix + ".bias", channels, err); if (!b) return fail(h, MP_EINVAL, err);
    BnLayer L;
    L.name = prefix; L.channels = channels;
    L.offset = h->bn_layers.empty() ? 0 : h->bn_layers.back().offset + 2LL * h->bn_layers.back().channels;
    int rc;
    if ((rc = upload(h, std::vector<float>(g, g + channels), &L.gamma))) return rc;
    if ((rc = upload(h, std::vector<float>(b, b + channels), &L.beta))) return rc;
    h->bn_layers.push_back(L);
    return MP_OK;
}

const char* kEncNames[7] = {"enc.conv2", "enc.conv3", "enc.conv4", "enc.conv5", "enc.conv6", "enc.conv7",
                            "enc.conv8"};

int build_encoder(mp_handle* h, TensorMap& tm, Encoder& E, const std::string& prefix)
{
    // MultiPoint: generate_encoder (MultiPoint.py:168-185): Sequential indices, 4 modules per conv block
    // (pad, conv, X, Y) and one MaxPool2d after blocks 2, 4, 6.
    // SuperPointMagicLeap (SuperPointMagicLeap.py:16-23): named convolutions, no BatchNorm.
    // double_convolution: false -- one (pad, conv, X, Y) group per stage, a pool after stages 1-3: indices 1, 6, 11, 16
    static const int conv_idx2[8] = {1, 5, 10, 14, 19, 23, 28, 32};
    static const int conv_idx1[4] = {1, 6, 11, 16};
    const bool dbl = h->cfg.double_convolution != 0;
    const int* conv_idx = dbl ? conv_idx2 : conv_idx1;
    static const char* ml_names[8] = {"conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b"};
    // MultiPoint.py:38-53: channel_version 0 [1,64,64,128,128], 1 [1,32,64,96,128], 2 [1,8,16,32,64]
    static const int stage_ch[3][5] = {{1, 64, 64, 128, 128}, {1, 32, 64, 96, 128}, {1, 8, 16, 32, 64}};
    const int* sc = stage_ch[h->cfg.channel_version];
    const int chan2[9] = {1, sc[1], sc[1], sc[2], sc[2], sc[3], sc[3], sc[4], sc[4]};
    const int chan1[9] = {1, sc[1], sc[2], sc[3], sc[4], 0, 0, 0, 0};
    const int* chan = dbl ? chan2 : chan1;
    // tensors carry zero padding channels up to a multiple of 32 (fp32 kernels) or 64 (fp16 kernels: their K chunk)
    const int pgran = h->cfg.mixed_precision ? 64 : 32;
    auto pad32 = [pgran](int c) { return ((c + pgran - 1) / pgran) * pgran; };
    static const bool pool2[8] = {false, true, false, true, false, true, false, false};
    static const bool pool1[8] = {true, true, true, false, false, false, false, false};
    const bool* pool = dbl ? pool2 : pool1;
    E.nconv = dbl ? 7 : 3;
    E.first_pool = pool[0];
    const int bn_off = h->cfg.bn_first ? 1 : 2;
    auto conv_key = [&](int i) {
        return h->cfg.key_layout == 1 ? std::string(ml_names[i]) : prefix + "." + std::to_string(conv_idx[i]);
    };
    auto bn_key = [&](int i) {
        return h->cfg.batchnorm ? prefix + "." + std::to_string(conv_idx[i] + bn_off) : std::string();
    };
    std::string err;
    // first layer (Cin = 1): [tap][cout], cout zero-padded to 32 / 64
    const int c1 = chan[1], c1p = pad32(c1);
    const float* w1 = tm.get(conv_key(0) + ".weight", c1 * 9, err); if (!w1) return fail(h, MP_EINVAL, err);
    const float* b1 = tm.get(conv_key(0) + ".bias", c1, err); if (!b1) return fail(h, MP_EINVAL, err);
    std::vector<float> wt(9 * c1p, 0.f), bias(c1p, 0.f), s1(c1p, 1.f), t1(c1p, 0.f);
    for (int co = 0; co < c1; ++co) {
        bias[co] = b1[co];
        for (int k = 0; k < 9; ++k) wt[k * c1p + co] = w1[co * 9 + k];
    }
    if (h->cfg.batchnorm && !bn_terms(tm, bn_key(0), c1, c1p, s1, t1, err)) return fail(h, MP_EINVAL, err);
    E.first.channels = c1p;
    int rc;
    if ((rc = upload(h, wt, &E.first.w))) return rc;
    if ((rc = upload(h, bias, &E.first.bias))) return rc;
    if ((rc = upload(h, s1, &E.first.scale))) return rc;
    if ((rc = upload(h, t1, &E.first.shift))) return rc;
    if (h->cfg.mixed_precision) {
        for (float& v : wt) v = round_half(v);
        for (float& v : bias) v = round_half(v);
        if ((rc = upload(h, wt, &E.first.w_h))) return rc;
        if ((rc = upload(h, bias, &E.first.bias_h))) return rc;
    }
    for (int i = 1; i <= E.nconv; ++i) {
        rc = build_conv(h, tm, E.conv[i - 1], kEncNames[i - 1], {conv_key(i)}, {bn_key(i)}, {chan[i + 1]}, pad32(chan[i]), 9,
                            pool[i], true, chan[i], true);
        if (rc) return rc;
    }
    for (int i = 0; i <= E.nconv && h->cfg.batchnorm; ++i) {
        rc = add_bn_layer(h, tm, bn_key(i), chan[i + 1]);
        if (rc) return rc;
    }
    // The fused F(4x4,3x3) conv1+conv2 launch (conv_wino43.hip F1: channel_version 0, double convolution, reflection padding) produces
    // relu(conv1) and nothing else per patch pixel: the first block's BatchNorm is folded at load time -- into the block's own weights
    // for bn_first models (conv -> BN -> ReLU), into conv2's Winograd-domain weights and bias otherwise (conv -> ReLU -> BN -> pad ->
    // conv2).  Exact in real arithmetic; in fp32 one rounding per activation fewer than the un-fused launches (equal within the tolerance
    // class of any two kernel variants: tests/test_gpu_parity.py::test_first_block_inside_f43_equals_standalone).
    if (dbl && h->cfg.channel_version == 0 && h->cfg.reflection_pad && E.conv[0].u43pack && E.conv[0].cin == 64 && chan[1] == 64) {
        const float* w2 = tm.get(conv_key(1) + ".weight", 64LL * 64 * 9, err); if (!w2) return fail(h, MP_EINVAL, err);
        const float* b2 = tm.get(conv_key(1) + ".bias", 64, err); if (!b2) return fail(h, MP_EINVAL, err);
        std::vector<float> wf(9 * 64), bf(64), b2f(64);
        const bool own = h->cfg.bn_first != 0;                      // fold into the block itself
        for (int co = 0; co < 64; ++co) {
            bf[co] = own ? (float)((double)b1[co] * s1[co] + t1[co]) : b1[co];
            for (int k = 0; k < 9; ++k) wf[k * 64 + co] = own ? (float)((double)w1[co * 9 + k] * s1[co]) : w1[co * 9 + k];
        }
        for (int o = 0; o < 64; ++o) {
            double acc = b2[o];
            if (!own)
                for (int c = 0; c < 64; ++c) {
                    double g = 0.0;
                    for (int k = 0; k < 9; ++k) g += w2[((size_t)o * 64 + c) * 9 + k];
                    acc += g * t1[c];
                }
            b2f[o] = (float)acc;
        }
        std::vector<float> u4;
        pack_wino43_weights({w2}, {64}, 64, 64, u4, own ? nullptr : s1.data());
        if ((rc = upload(h, wf, &E.first.w_f1))) return rc;
        if ((rc = upload(h, bf, &E.first.bias_f1))) return rc;
        if ((rc = upload(h, u4, &E.conv[0].u43pack_f1))) return rc;
        if ((rc = upload(h, b2f, &E.conv[0].bias_f1))) return rc;
    }
    return MP_OK;
}

// the convolution algorithm of the 3x3 layers is a MODEL setting (yaml model.conv_algorithm: 0 auto, 1 winograd43, 2
// winograd43_general, 3 direct); the MP_DEBUG switches only choose for 'auto'.  batch_invariant: never split the input channels
ConvPolicy conv_policy(const DebugSwitches& d, const mp_model_config& cfg)
{
    ConvPolicy p;
    p.direct = cfg.conv_algorithm == 3 || (cfg.conv_algorithm == 0 && !d.winograd);
    p.wino43 = !p.direct && (cfg.conv_algorithm != 0 || d.wino43);
    p.wino43_gen = cfg.conv_algorithm == 1 ? 0 : cfg.conv_algorithm == 2 ? 2 : d.wino43_gen;
    p.splitk_max = cfg.batch_invariant ? 1 : d.splitk_max;
    return p;
}

}  // namespace

extern "C" {

int mp_load_weights(mp_handle* h, const mp_model_config* cfg, const mp_tensor* tensors, int n_tensors)
{
    if (!h) return MP_EINVAL;
    if (!cfg || (!tensors && n_tensors > 0)) return fail(h, MP_EINVAL, "mp_load_weights: NULL argument");
    if (cfg->channel_version < 0 || cfg->channel_version > 2)
        return fail(h, MP_EINVAL, "unsupported model config: channel_version must be 0, 1 or 2 (MultiPoint.py:38-53)");
    if (cfg->channel_version != 0 && cfg->key_layout == 1)
        return fail(h, MP_EINVAL, "unsupported model config: SuperPointMagicLeap has channel_version 0 shapes");
    if (!cfg->double_convolution && cfg->key_layout == 1)
        return fail(h, MP_EINVAL, "unsupported model config: SuperPointMagicLeap has two convolutions per stage");
    if (cfg->descriptor_head && cfg->descriptor_size != 64 && cfg->descriptor_size != 128 &&
        cfg->descriptor_size != 256)
        return fail(h, MP_EINVAL, "unsupported model config: descriptor_size must be 64, 128 or 256");
    if (cfg->conv_algorithm < 0 || cfg->conv_algorithm > 3)
        return fail(h, MP_EINVAL, "unsupported model config: conv_algorithm must be 0 (auto), 1 (winograd43), 2 (winograd43_general) or 3 (direct)");
    MP_HIP(hipSetDevice(h->device));
    free_weights(h);
    h->cfg = *cfg;
    h->policy = conv_policy(h->dbg, *cfg);
    TensorMap tm;
    for (int i = 0; i < n_tensors; ++i) {
        if (!tensors[i].name || (!tensors[i].data && tensors[i].numel > 0))
            return fail(h, MP_EINVAL, "mp_load_weights: tensor " + std::to_string(i) + " has NULL field");
        tm.m[tensors[i].name] = &tensors[i];
    }
    int rc;
    if (cfg->key_layout == 1 && (cfg->multispectral || cfg->batchnorm || cfg->final_batchnorm))
        return fail(h, MP_EINVAL, "unsupported model config: SuperPointMagicLeap key layout has one encoder and no BatchNorm");
    if (!cfg->batchnorm && cfg->key_layout == 0)
        return fail(h, MP_EINVAL, "unsupported model config: MultiPoint key layout always has BatchNorm2d");
    if (cfg->multispectral) {
        if ((rc = build_encoder(h, tm, h->enc[0], "encoder_thermal"))) return rc;
        if ((rc = build_encoder(h, tm, h->enc[1], "encoder_optical"))) return rc;
    } else {
        if ((rc = build_encoder(h, tm, h->enc[0], "encoder"))) return rc;
    }
    // head key names: MultiPoint nn.Sequential (MultiPoint.py:62-88) or SuperPointMagicLeap (:25-29)
    const bool ml = cfg->key_layout == 1;
    const std::string det = "detector_head_convolutions", dsc = "descriptor_head_convolutions";
    const std::string bn3 = cfg->bn_first ? ".2" : ".3";
    const std::string det3 = ml ? "convPa" : det + ".1", dsc3 = ml ? "convDa" : dsc + ".1";
    const std::string det1k = ml ? "convPb" : det + ".4", dsc1k = ml ? "convDb" : dsc + ".4";
    const std::string det3bn = cfg->batchnorm ? det + bn3 : std::string(), dsc3bn = cfg->batchnorm ? dsc + bn3 : std::string();
    const std::string det1bn = cfg->final_batchnorm ? det + ".5" : std::string();
    const std::string dsc1bn = cfg->final_batchnorm ? dsc + ".5" : std::string();
    // both 3x3 head convs read the same encoder output: one launch with N = hc (+hc); hc = 256 for channel_version 0,
    // descriptor_size otherwise (MultiPoint.py:38-53)
    const int hc = cfg->channel_version == 0 ? 256 : cfg->descriptor_size;
    const int enc_out = h->enc[0].conv[h->enc[0].nconv - 1].cout;                 // 128 (64 for channel_version 2)
    const int enc_real = cfg->channel_version == 2 ? 64 : 128;
    h->head_channels = hc;
    if (cfg->descriptor_head)
        rc = build_conv(h, tm, h->heads3, "heads.conv3x3", {det3, dsc3}, {det3bn, dsc3bn}, {hc, hc}, enc_out, 9, false, true, enc_real);
    else
        rc = build_conv(h, tm, h->heads3, "heads.conv3x3", {det3}, {det3bn}, {hc}, enc_out, 9, false, true, enc_real);
    if (rc) return rc;
    if ((rc = build_conv(h, tm, h->det1, "det.conv1x1", {det1k}, {det1bn}, {65}, hc, 1, false, false))) return rc;
    if (cfg->descriptor_head &&
        (rc = build_conv(h, tm, h->desc1, "desc.conv1x1", {dsc1k}, {dsc1bn}, {cfg->descriptor_size}, hc, 1, false, false)))
        return rc;
    if (cfg->batchnorm) {           // the heads' BatchNorm layers, state_dict order: detector (3x3, final), descriptor (3x3, final)
        if ((rc = add_bn_layer(h, tm, det3bn, hc))) return rc;
        if (cfg->final_batchnorm && (rc = add_bn_layer(h, tm, det1bn, 65))) return rc;
        if (cfg->descriptor_head && (rc = add_bn_layer(h, tm, dsc3bn, hc))) return rc;
        if (cfg->descriptor_head && cfg->final_batchnorm && (rc = add_bn_layer(h, tm, dsc1bn, cfg->descriptor_size))) return rc;
        std::vector<float> ident(1024, 0.f);
        for (int i = 0; i < 512; ++i) ident[i] = 1.f;
        if ((rc = upload(h, ident, &h->bn_ident))) return rc;
    }
    // strict=True semantics of load_state_dict: no unexpected keys
    for (auto& kv : tm.m)
        if (!tm.used.count(kv.first)) {
            if (kv.first.size() > 20 && kv.first.rfind(".num_batches_tracked") == kv.first.size() - 20) continue;
            free_weights(h);
            return fail(h, MP_EINVAL, "unexpected key in state_dict: " + kv.first);
        }
    h->loaded = true;
    return MP_OK;
}

}  // extern "C"
