// C ABI of libmultipoint_hip.so (declared in include/multipoint_hip.h): the handle's life cycle, the device shape, the MP_DEBUG
// switches and profiling.  The model is loaded in model_load.hip, the forward runs in forward.hip, the rest of the ABI is
// post_api.hip and the *_api.hip files; host.h holds the handle.
#include "host.h"

using namespace mp_host;

namespace {

// MP_DEBUG: the ONE environment variable the library reads (in mp_create), a comma-separated list of developer switches
// `key` or `key=value` -- kernel selection for A/B runs and for the parity tests, which hold every kernel variant to the CPU reference path.
// They are not configuration: a model's algorithm is `model.conv_algorithm` / `model.batch_invariant` (mp_model_config).
//   no_winograd          the direct implicit-GEMM kernels for every 3x3 layer (what conv_algorithm 3 selects per model)
//   wino43=0             F(4x4,3x3) for no layer (round 6 retired the value 1 = 64-input-channel layers only: no routing selects it)
//   wino43_gen=0|1|2     0 conv_wino43.hip where it applies and conv_wino43b.hip elsewhere; 1 / 2: only that kernel
//   no_fuse              the fp32 first block as its own launch in front of the direct conv2 kernel
//   no_fuse43            ... in front of the F(4x4,3x3) conv2 kernel
//   no_head_fuse         separate 1x1 convolution / softmax / normalisation launches instead of the fused head tail (fp32 and fp16)
//   no_vin               the 3x3 head convolutions (>= 4 output slices) transform their input per slice inside the kernel instead of
//                        taking it pre-transformed from a pass of its own (conv_wino43.hip VIN; bit-identical either way)
//   no_planar            channel-quad-planar tensors never (default: behind conv1 and pooled producers; round 6 retired planar=2 = everywhere)
//   no_xplanar           column-interleaved planar tensors never: the tensors between an un-pooled conv_wino43.hip launch and its
//                        conv_wino43.hip consumer stay NHWC (bit-identical either way; no_planar implies it)
//   no_persist, persist_min_items=N   direct kernels: per-tile launches / persistent from N items per CU
//   splitk_max=1..8      most ranges the input channels of a small launch are cut into
//   f16_no_res, f16_no_fuse1, f16_res_groups=2   fp16 path: streaming kernel everywhere / first block as its own launch / two groups
//   ncu=N, nxcd=N        emulate a partitioned device (fewer persistent workgroups, same results)
// Returns true when `key` is present; *value receives the integer behind '=' (or `dflt` for a bare key).
bool debug_switch(const char* key, int* value = nullptr, int dflt = 1)
{
    const char* e = getenv("MP_DEBUG");
    if (!e) return false;
    const size_t kl = std::strlen(key);
    for (const char* q = e; *q;) {
        while (*q == ',' || *q == ' ') ++q;
        const char* end = q;
        while (*end && *end != ',') ++end;
        if ((size_t)(end - q) >= kl && std::strncmp(q, key, kl) == 0 && (q[kl] == '=' || q + kl == end || q[kl] == ' ')) {
            if (value) *value = q[kl] == '=' ? atoi(q + kl + 1) : dflt;
            return true;
        }
        q = end;
    }
    return false;
}

// XCC (= XCD) count of the KFD topology node whose PCI location matches `bus_id` ("dddd:bb:dd.f"); 0 if the topology is not
// readable (containers without /sys/class/kfd): the caller then falls back to compute units / 32
int kfd_num_xcc(const char* bus_id)
{
    unsigned dom = 0, bus = 0, dev = 0, fn = 0;
    if (sscanf(bus_id, "%x:%x:%x.%x", &dom, &bus, &dev, &fn) != 4) return 0;
    const unsigned long long want = ((unsigned long long)bus << 8) | (dev << 3) | fn;
    for (int node = 0; node < 64; ++node) {
        char path[128];
        snprintf(path, sizeof path, "/sys/class/kfd/kfd/topology/nodes/%d/properties", node);
        FILE* f = fopen(path, "r");
        if (!f) { if (node > 8) break; else continue; }
        char key[64]; unsigned long long val = 0, loc = ~0ull, domain = 0, xcc = 0, simd = 0;
        while (fscanf(f, "%63s %llu", key, &val) == 2) {
            if (!strcmp(key, "location_id")) loc = val;
            else if (!strcmp(key, "domain")) domain = val;
            else if (!strcmp(key, "num_xcc")) xcc = val;
            else if (!strcmp(key, "simd_count")) simd = val;
        }
        fclose(f);
        if (simd > 0 && loc == want && domain == dom) return (int)xcc;
    }
    return 0;
}

}  // namespace

extern "C" {

const char* mp_version(void) { return "multipoint_hip 0.1 (gfx950)"; }

const char* mp_last_error(const mp_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int mp_device_shape(const mp_handle* h, int* compute_units, int* xcds, int* persistent_workgroups)
{
    if (!h) return MP_EINVAL;
    if (compute_units) *compute_units = h->ncu;
    if (xcds) *xcds = 1 << h->xcd_shift;
    if (persistent_workgroups) *persistent_workgroups = (int)persistent_grid(1ll << 40, h->ncu, h->xcd_shift);
    return MP_OK;
}

int mp_create(mp_handle** out, int device)
{
    mp_handle* h = nullptr;
    if (!out) return fail(h, MP_EINVAL, "mp_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    MP_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return fail(h, MP_EINVAL, "mp_create: device " + std::to_string(device) + " not available (" +
                                      std::to_string(ndev) + " HIP devices visible)");
    MP_HIP(hipSetDevice(device));
    {
        // Rounds 1-4 read ~20 MP_* kernel-selection variables; round 5 folded them into MP_DEBUG=key[=value],... .  A script that
        // still sets an old name would silently A/B the default against itself: say so once.
        static const char* const legacy[] = {"MP_NO_WINOGRAD", "MP_WINO43", "MP_WINO43_GEN", "MP_NO_FUSE", "MP_NO_FUSE43", "MP_NO_HEAD_FUSE",
            "MP_NO_PLANAR", "MP_PLANAR", "MP_NO_PERSIST", "MP_PERSIST_MIN_ITEMS", "MP_SPLITK_MAX", "MP_F16_NO_RES", "MP_F16_NO_FUSE1",
            "MP_F16_RES_GROUPS", "MP_NCU", "MP_NXCD", "MP_POST_OVERLAP", "MP_NO_VIN", "MP_NO_POOL_FIRST"};
        static bool warned = false;
        for (const char* k : legacy)
            if (!warned && getenv(k)) {
                warned = true;
                fprintf(stderr, "libmultipoint_hip: the environment variable %s is no longer read (nor are the other MP_* kernel switches): "
                                "use MP_DEBUG=key[=value],... -- the keys are listed in csrc/api.hip (debug_switch)\n", k);
            }
    }
    hipDeviceProp_t prop;
    MP_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(h, MP_EINVAL, std::string("mp_create: kernels are built for gfx950 only, device is ") +
                                      prop.gcnArchName);
    // Machine shape: every persistent kernel launches one (fp16: two) workgroup(s) per compute unit and walks, per XCD, a
    // contiguous share of the work items (workgroup b is dispatched to XCD b mod nxcd; each XCD has its own L2).  Both numbers
    // come from the device: multiProcessorCount, and the XCC count of the KFD topology node at the device's PCI address
    // (a partitioned MI355X -- DPX / QPX / CPX -- reports 4 / 2 / 1 XCDs with 128 / 64 / 32 CUs).  MP_DEBUG=ncu / MP_DEBUG=nxcd override
    // (tests emulate smaller partitions on the full device: fewer workgroups, same results).
    int ncu = prop.multiProcessorCount, nxcd = 0;
    {
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, sizeof bus, device) == hipSuccess) nxcd = kfd_num_xcc(bus);
        if (nxcd <= 0) nxcd = ncu >= 32 ? ncu / 32 : 1;           // gfx950: 32 active CUs per XCD
        int v = 0;
        if (debug_switch("ncu", &v) && v > 0 && v <= ncu) ncu = v;
        if (debug_switch("nxcd", &v) && v > 0) nxcd = v;
    }
    if (ncu < 1 || nxcd < 1 || (nxcd & (nxcd - 1)) != 0 || nxcd > ncu)
        return fail(h, MP_EINVAL, "mp_create: unsupported machine shape: " + std::to_string(ncu) + " compute units in " +
                                      std::to_string(nxcd) + " XCDs (the XCD count must be a power of two <= the CU count)");
    int xcd_shift = 0;
    while ((1 << xcd_shift) < nxcd) ++xcd_shift;
    DebugSwitches d;                                          // every other MP_DEBUG key
    int v = 0;
    d.winograd = !debug_switch("no_winograd");
    if (debug_switch("wino43", &v) && v == 0) d.wino43 = false;
    if (debug_switch("wino43_gen", &v) && v >= 0 && v <= 2) d.wino43_gen = v;
    d.fuse_first = !debug_switch("no_fuse");
    d.fuse43 = !debug_switch("no_fuse43");
    d.head_fuse = !debug_switch("no_head_fuse");
    d.vin = !debug_switch("no_vin");
    d.planar = !debug_switch("no_planar");
    d.xplanar = d.planar && !debug_switch("no_xplanar");
    if (debug_switch("persist_min_items", &v) && v > 0) d.persist = v;
    if (debug_switch("no_persist")) d.persist = 0;
    if (debug_switch("splitk_max", &v) && v >= 1 && v <= 8) d.splitk_max = v;
    d.f16_res = !debug_switch("f16_no_res");
    d.f16_fuse1 = !debug_switch("f16_no_fuse1");
    if (debug_switch("f16_res_groups", &v) && v == 2) d.f16_res_groups = 2;
    mp_handle* hh = new mp_handle(device, ncu, xcd_shift, d);
    if (hipHostMalloc(reinterpret_cast<void**>(&hh->pinned), 4096) != hipSuccess) {
        delete hh;
        return fail(h, MP_ENOMEM, "mp_create: hipHostMalloc failed");
    }
    *out = hh;
    return MP_OK;
}

void mp_destroy(mp_handle* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    int* pinned = h->pinned;
    const std::vector<ProfEntry> events = std::move(h->prof_entries);
    delete h;                       // its DevBufs free the device memory
    if (pinned) (void)hipHostFree(pinned);
    for (auto& e : events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
}

int mp_profile_enable(mp_handle* h, int enable)
{
    if (!h) return MP_EINVAL;
    h->prof = enable != 0;
    h->prof_used = 0;
    return MP_OK;
}

int mp_profile_read(mp_handle* h, const char** names, float* ms, double* flop, int capacity, int* n)
{
    if (!h || !n) return MP_EINVAL;
    *n = 0;
    for (size_t i = 0; i < h->prof_used && (int)i < capacity; ++i) {
        ProfEntry& e = h->prof_entries[i];
        MP_HIP(hipEventSynchronize(e.b));
        float t = 0.f;
        MP_HIP(hipEventElapsedTime(&t, e.a, e.b));
        if (names) names[i] = e.name;
        if (ms) ms[i] = t;
        if (flop) flop[i] = e.flop;
        ++*n;
    }
    h->prof_used = 0;
    return MP_OK;
}

}  // extern "C"
