// libhrt.so -- C ABI (include/hrt.h) over the HIP kernels in hrt_kernels.hip.
// gfx950 only.  No CPU fallback: every entry point that needs the GPU fails
// with HRT_ERR_DEVICE when HIP cannot provide one.
#include "hrt_kernels.hip"
#include "hrt_dual.hip"
#include "hrt_stream.hip"
#include "hrt_output.hip"
#include "hrt_kat.hip"
#include "hrt_pack.h"  // hrt_scene_desc -> host arrays (pack_scene): everything of scene creation that needs no device
#include "hrt_bake_points.h"  // the host-only bake point generators (hrt_bake_quad_points, hrt_bake_mesh_points)
#include "hrt_probe_points.h"  // the host-only probe grid generator (hrt_probe_grid_points)
#include "hrt_probe_volume_cell.h"  // the cell and the weights of a probe volume, for the host and the device (with hrt_probe_depth_oct.h, the octahedral depth map)

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl.so is opened with dlopen by hrt_multi_create (hrt_multi.hip)

#include <array>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {

thread_local std::string g_error;
int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(HRT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

// The HRT_KERNEL environment variable: "single", "dual", "stream", or anything else for the default.
struct KernelPref {
    bool use_dual = true;  // two pixel streams per lane (hrt_dual.hip) for scenes with meshes; "single" turns it off
    int use_stream = -1;   // workgroup-streaming kernel (hrt_stream.hip): -1 where it pays (default), 1 always ("stream"), 0 never
};
KernelPref parse_kernel_pref(const char *k) {
    const std::string ks = k ? k : "";
    return KernelPref{ks != "single", ks == "stream" ? 1 : ((ks == "single" || ks == "dual") ? 0 : -1)};
}

struct Runtime {
    bool ready = false;
    int device = -1;
    int cus = 0;
    int blocks_per_cu = 0;
    uint32_t lds_budget = 0;  // bytes of dynamic LDS per workgroup for nodelets
    KernelPref pref;          // what HRT_KERNEL asks for
    hipFuncAttributes attr{};
    std::vector<int> dev_cus;  // per ordinal: CUs of the devices hrt_init has prepared (0 = not prepared); one process may drive several
} g_rt;

// Makes `ordinal` (a device hrt_init has prepared) the current one for this thread and for the launch geometry.
int use_device(int ordinal) {
    if (ordinal < 0 || ordinal >= (int)g_rt.dev_cus.size() || g_rt.dev_cus[ordinal] == 0)
        return fail(HRT_ERR_STATE, "device " + std::to_string(ordinal) + " has not been initialised (hrt_init)");
    HIP_TRY(hipSetDevice(ordinal));
    g_rt.device = ordinal;
    g_rt.cus = g_rt.dev_cus[ordinal];
    return HRT_OK;
}

// host fp64 helpers of the camera, in the reference's evaluation order (no contraction)
double h_mul64(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
double h_neg_dot3(const double r[3], const float e[3]) {  // -(r . e), left to right, no contraction (as oracle/oracle.cpp builds it)
#pragma clang fp contract(off)
    return -(r[0] * (double)e[0] + r[1] * (double)e[1] + r[2] * (double)e[2]);
}
// gluInvertMatrix (matrixUtilities.h:77-206): adjugate over determinant.  Each adjugate entry is six signed triple
// products ((s*m[a]) * m[b]) * m[c] summed in the order listed, which is the order the reference writes them in, so
// every entry rounds as the reference's.
static const signed char k_adjugate[16][6][4] = {
    {{1, 5, 10, 15}, {-1, 5, 11, 14}, {-1, 9, 6, 15}, {1, 9, 7, 14}, {1, 13, 6, 11}, {-1, 13, 7, 10}},
    {{-1, 1, 10, 15}, {1, 1, 11, 14}, {1, 9, 2, 15}, {-1, 9, 3, 14}, {-1, 13, 2, 11}, {1, 13, 3, 10}},
    {{1, 1, 6, 15}, {-1, 1, 7, 14}, {-1, 5, 2, 15}, {1, 5, 3, 14}, {1, 13, 2, 7}, {-1, 13, 3, 6}},
    {{-1, 1, 6, 11}, {1, 1, 7, 10}, {1, 5, 2, 11}, {-1, 5, 3, 10}, {-1, 9, 2, 7}, {1, 9, 3, 6}},
    {{-1, 4, 10, 15}, {1, 4, 11, 14}, {1, 8, 6, 15}, {-1, 8, 7, 14}, {-1, 12, 6, 11}, {1, 12, 7, 10}},
    {{1, 0, 10, 15}, {-1, 0, 11, 14}, {-1, 8, 2, 15}, {1, 8, 3, 14}, {1, 12, 2, 11}, {-1, 12, 3, 10}},
    {{-1, 0, 6, 15}, {1, 0, 7, 14}, {1, 4, 2, 15}, {-1, 4, 3, 14}, {-1, 12, 2, 7}, {1, 12, 3, 6}},
    {{1, 0, 6, 11}, {-1, 0, 7, 10}, {-1, 4, 2, 11}, {1, 4, 3, 10}, {1, 8, 2, 7}, {-1, 8, 3, 6}},
    {{1, 4, 9, 15}, {-1, 4, 11, 13}, {-1, 8, 5, 15}, {1, 8, 7, 13}, {1, 12, 5, 11}, {-1, 12, 7, 9}},
    {{-1, 0, 9, 15}, {1, 0, 11, 13}, {1, 8, 1, 15}, {-1, 8, 3, 13}, {-1, 12, 1, 11}, {1, 12, 3, 9}},
    {{1, 0, 5, 15}, {-1, 0, 7, 13}, {-1, 4, 1, 15}, {1, 4, 3, 13}, {1, 12, 1, 7}, {-1, 12, 3, 5}},
    {{-1, 0, 5, 11}, {1, 0, 7, 9}, {1, 4, 1, 11}, {-1, 4, 3, 9}, {-1, 8, 1, 7}, {1, 8, 3, 5}},
    {{-1, 4, 9, 14}, {1, 4, 10, 13}, {1, 8, 5, 14}, {-1, 8, 6, 13}, {-1, 12, 5, 10}, {1, 12, 6, 9}},
    {{1, 0, 9, 14}, {-1, 0, 10, 13}, {-1, 8, 1, 14}, {1, 8, 2, 13}, {1, 12, 1, 10}, {-1, 12, 2, 9}},
    {{-1, 0, 5, 14}, {1, 0, 6, 13}, {1, 4, 1, 14}, {-1, 4, 2, 13}, {-1, 12, 1, 6}, {1, 12, 2, 5}},
    {{1, 0, 5, 10}, {-1, 0, 6, 9}, {-1, 4, 1, 10}, {1, 4, 2, 9}, {1, 8, 1, 6}, {-1, 8, 2, 5}}};
bool host_invert4(const double m[16], double out[16]) {
#pragma clang fp contract(off)
    double adj[16];
    for (int e = 0; e < 16; ++e) {
        double sum = 0.0;
        for (int k = 0; k < 6; ++k) {
            const signed char *t = k_adjugate[e][k];
            const double term = ((t[0] < 0 ? -m[t[1]] : m[t[1]]) * m[t[2]]) * m[t[3]];
            sum = k == 0 ? term : sum + term;
        }
        adj[e] = sum;
    }
    double det = m[0] * adj[0] + m[1] * adj[4] + m[2] * adj[8] + m[3] * adj[12];
    if (det == 0) return false;
    det = 1.0 / det;
    for (int e = 0; e < 16; ++e) out[e] = adj[e] * det;
    return true;
}

// ---- The owners.  Every HIP resource the library holds belongs to exactly one of these four, which acquires it, frees it in its
// destructor (or in release(), for whoever must choose the device that is current at that moment: hrt_multi_destroy) and counts it
// in g_live (hrt_debug_live_resources).  All are move-only.  An error return (HIP_TRY) may therefore leave any scope that holds
// them.  NONE MAY HAVE STATIC STORAGE DURATION: the HIP runtime may be gone by the time static destructors run.
enum { LIVE_DEVICE, LIVE_PINNED, LIVE_EVENT, LIVE_STREAM };
std::atomic<uint64_t> g_live[4];  // plain counters: nothing to destroy

// A device buffer that grows on demand and never shrinks; the capacity is in bytes.  The old block is freed before the larger one
// is asked for (its contents are never wanted), so a frame size that only just fits does not need both at once.
struct Scratch {
    void *p = nullptr;
    size_t cap = 0;
    Scratch() = default;
    Scratch(Scratch &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { release(); }
    template <class T> T *as() const { return (T *)p; }
    void release() {
        if (p) { (void)hipFree(p); --g_live[LIVE_DEVICE]; }
        p = nullptr; cap = 0;
    }
    int grow(size_t bytes) {
        if (cap >= bytes) return HRT_OK;
        release();
        HIP_TRY(hipMalloc(&p, bytes));
        ++g_live[LIVE_DEVICE];
        cap = bytes;
        return HRT_OK;
    }
    // Room for n elements of T, and for one where n is 0: an empty array still has an address.
    template <class T> int need(size_t n) { return grow(std::max<size_t>(n, 1) * sizeof(T)); }
    // Room for `bytes` (need's rule is the caller's), filled from host memory with a blocking copy.
    int from_host(const void *src, size_t bytes) {
        if (const int rc = grow(bytes)) return rc;
        if (bytes) HIP_TRY(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        return HRT_OK;
    }
};

// A pinned host buffer, grown as Scratch grows.
struct Pinned {
    void *p = nullptr;
    size_t cap = 0;
    Pinned() = default;
    Pinned(Pinned &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Pinned(const Pinned &) = delete;
    Pinned &operator=(const Pinned &) = delete;
    ~Pinned() { release(); }
    void release() {
        if (p) { (void)hipHostFree(p); --g_live[LIVE_PINNED]; }
        p = nullptr; cap = 0;
    }
    int grow(size_t bytes) {
        if (cap >= bytes) return HRT_OK;
        release();
        HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        ++g_live[LIVE_PINNED];
        cap = bytes;
        return HRT_OK;
    }
};

// An event, created by the first ready(flags) and handed to HIP as the handle it holds.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { release(); }
    operator hipEvent_t() const { return e; }
    void release() {
        if (e) { (void)hipEventDestroy(e); --g_live[LIVE_EVENT]; }
        e = nullptr;
    }
    int ready(unsigned flags = hipEventDefault) {  // the default times (a timing pair); hipEventDisableTiming orders only
        if (e) return HRT_OK;
        HIP_TRY(hipEventCreateWithFlags(&e, flags));
        ++g_live[LIVE_EVENT];
        return HRT_OK;
    }
};

// A stream of the library's own.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { release(); }
    operator hipStream_t() const { return s; }
    void release() {
        if (s) { (void)hipStreamDestroy(s); --g_live[LIVE_STREAM]; }
        s = nullptr;
    }
    int ready(unsigned flags) {
        if (s) return HRT_OK;
        HIP_TRY(hipStreamCreateWithFlags(&s, flags));
        ++g_live[LIVE_STREAM];
        return HRT_OK;
    }
};

// The last launch that read a buffer of a scene's, for whoever writes or frees that buffer next.  Launches on one stream are ordered
// by the stream; a writer on another stream first waits for `done` there (wait_on), and the host waits for it before the buffer
// is freed (sync).
struct LastReader {
    Event done;
    bool used = false;
    hipStream_t stream = nullptr;  // of the reader
    int ready() { return done.ready(hipEventDisableTiming); }
    int wait_on(hipStream_t on) {  // before the first write enqueued on `on`
        if (const int rc = ready()) return rc;
        if (used && stream != on) HIP_TRY(hipStreamWaitEvent(on, done, 0));
        return HRT_OK;
    }
    int sync() {  // host wait, before the buffer is freed
        if (used) HIP_TRY(hipEventSynchronize(done));
        return HRT_OK;
    }
    int mark(hipStream_t on) {  // after the launch on `on` that reads the buffer
        HIP_TRY(hipEventRecord(done, on));
        used = true;
        stream = on;
        return HRT_OK;
    }
};

// A per-launch table of T in device memory that a call fills from the host: a grow-only device table, its pinned staging copy (the
// caller's entries are free when the call returns) with the event that says the upload has read it, and the table's last reader.
// T may be incomplete where the table is declared.  stage() is the whole sequence; the trace path (hrt_views.hip) runs its parts
// itself, because its upload belongs behind launch_trace's own cross-stream wait.
template <class T>
struct StagedTable {
    Scratch dev;
    Pinned host;
    Event uploaded;
    bool uploading = false;
    LastReader reader;
    const T *table() const { return dev.as<T>(); }
    // The entries into the staging copy and room for them on the device.  The staging copy is reused by every call: wait until
    // the previous call's upload has read it (that upload sits in front of its kernel, so this does not wait for the kernel).
    // sync_reader: the host waits for the table's last reader before a larger table replaces (frees) the old one.  false only where
    // the caller's launches are ordered behind one another by other means.
    int fill(const std::vector<T> &entries, bool sync_reader) {
        const size_t bytes = entries.size() * sizeof(T);
        if (uploading) { HIP_TRY(hipEventSynchronize(uploaded)); uploading = false; }
        if (const int rc = uploaded.ready(hipEventDisableTiming)) return rc;
        if (const int rc = reader.ready()) return rc;
        if (const int rc = host.grow(bytes)) return rc;
        std::memcpy(host.p, entries.data(), bytes);
        if (sync_reader && dev.cap < bytes)
            if (const int rc = reader.sync()) return rc;
        return dev.grow(bytes);
    }
    // The staged entries to the device on `stream`, behind whatever the caller has made `stream` wait for.
    int upload(size_t n, hipStream_t stream) {
        HIP_TRY(hipMemcpyAsync(dev.p, host.p, n * sizeof(T), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(uploaded, stream));
        uploading = true;
        return HRT_OK;
    }
    // fill, wait on `stream` for a last reader on another stream, upload: *out is ready for a launch on `stream`, which staged() follows.
    int stage(const std::vector<T> &entries, hipStream_t stream, const T **out) {
        int rc = fill(entries, true);
        if (rc == HRT_OK) rc = reader.wait_on(stream);
        if (rc == HRT_OK) rc = upload(entries.size(), stream);
        *out = table();
        return rc;
    }
    int staged(hipStream_t stream) { return reader.mark(stream); }
};

// w x h is a frame of at most max_pixels pixels (2^31 - 1 where pixels are indexed, 2^31 / 16 where 16-byte records of them are).
int check_frame(const std::string &who, uint32_t w, uint32_t h, uint64_t max_pixels) {
    if (!w || !h) return fail(HRT_ERR_INVALID, who + ": w and h must be positive (got " + std::to_string(w) + " x " + std::to_string(h) + ")");
    if ((uint64_t)w * h > max_pixels) return fail(HRT_ERR_INVALID, who + ": image too large: w * h must be at most " + std::to_string(max_pixels));
    return HRT_OK;
}
const uint64_t k_max_pixels = 0x7fffffffull, k_max_records = 0x7fffffffull / 16u;

// The margin scale of the filters (CtxT::err_abs) for rays of unit direction that start |o| from the world origin in a scene whose
// points lie within `bound` of it.
__host__ __device__ __forceinline__ float margin_scale(float bound, float olen) { return 2e-6f * (bound + olen + 1.f); }

// HRT_FLAG_MESH_BRUTE exists in the proof builds only.
int check_mesh_brute(const std::string &who, uint32_t flags) {
    if ((flags & HRT_FLAG_MESH_BRUTE) && !(flags & HRT_FLAG_EXACT_ONLY)) return fail(HRT_ERR_INVALID, who + ": flags: HRT_FLAG_MESH_BRUTE needs HRT_FLAG_EXACT_ONLY");
    return HRT_OK;
}

// ---- The builds of the trace kernels, stated once: hrt_init raises every row's dynamic-LDS limit,
// pick_build chooses a row, launch_trace sizes and launches it.  tests/test_kernel_choice.py holds the table to the sources.
enum KernelFamily { KF_LANE, KF_DUAL, KF_STREAM };  // lane-per-pixel (hrt_kernels.hip), two-stream (hrt_dual.hip), workgroup-streaming (hrt_stream.hip)
enum : uint32_t { KB_LIGHTS = 1u, KB_EXACT = 2u, KB_SPH = 4u, KB_LIST = 8u, KB_VIEWS = 16u };  // lights, proof, sphere pair filter, tile list, batched views
struct KernelBuild {
    KernelFamily family; uint32_t bits; void (*fn)(const DRender); const char *name;
    uint32_t wg() const { return family == KF_STREAM ? HRT_SP_WG : HRT_WG; }  // threads per workgroup
};
#define HRT_BUILD(k, family, bits) {family, bits, k, #k}
const KernelBuild k_builds[] = {
    HRT_BUILD(hrt_trace_kernel, KF_LANE, 0u),
    HRT_BUILD(hrt_trace_kernel_lights, KF_LANE, KB_LIGHTS),
    HRT_BUILD(hrt_trace_kernel_exact, KF_LANE, KB_EXACT),
    HRT_BUILD(hrt_trace_kernel_lights_exact, KF_LANE, KB_LIGHTS | KB_EXACT),
    HRT_BUILD(hrt_trace_kernel_list, KF_LANE, KB_LIST),
    HRT_BUILD(hrt_trace_kernel_lights_list, KF_LANE, KB_LIGHTS | KB_LIST),
    HRT_BUILD(hrt_trace_kernel_exact_list, KF_LANE, KB_EXACT | KB_LIST),
    HRT_BUILD(hrt_trace_kernel_lights_exact_list, KF_LANE, KB_LIGHTS | KB_EXACT | KB_LIST),
    HRT_BUILD(hrt_trace_kernel_views, KF_LANE, KB_VIEWS),
    HRT_BUILD(hrt_trace_kernel_lights_views, KF_LANE, KB_LIGHTS | KB_VIEWS),
    HRT_BUILD(hrt_trace2_kernel, KF_DUAL, 0u),
    HRT_BUILD(hrt_trace2_kernel_lights, KF_DUAL, KB_LIGHTS),
    HRT_BUILD(hrt_trace2_kernel_list, KF_DUAL, KB_LIST),
    HRT_BUILD(hrt_trace2_kernel_lights_list, KF_DUAL, KB_LIGHTS | KB_LIST),
    HRT_BUILD(hrt_wgstream_kernel, KF_STREAM, 0u),
    HRT_BUILD(hrt_wgstream_kernel_lights, KF_STREAM, KB_LIGHTS),
    HRT_BUILD(hrt_wgstream_kernel_sph, KF_STREAM, KB_SPH),
    HRT_BUILD(hrt_wgstream_kernel_lights_sph, KF_STREAM, KB_LIGHTS | KB_SPH),
    HRT_BUILD(hrt_wgstream_kernel_exact, KF_STREAM, KB_EXACT),
    HRT_BUILD(hrt_wgstream_kernel_lights_exact, KF_STREAM, KB_LIGHTS | KB_EXACT),
    HRT_BUILD(hrt_wgstream_kernel_list, KF_STREAM, KB_LIST),
    HRT_BUILD(hrt_wgstream_kernel_lights_list, KF_STREAM, KB_LIGHTS | KB_LIST),
    HRT_BUILD(hrt_wgstream_kernel_sph_list, KF_STREAM, KB_SPH | KB_LIST),
    HRT_BUILD(hrt_wgstream_kernel_lights_sph_list, KF_STREAM, KB_LIGHTS | KB_SPH | KB_LIST),
    HRT_BUILD(hrt_wgstream_kernel_exact_list, KF_STREAM, KB_EXACT | KB_LIST),
    HRT_BUILD(hrt_wgstream_kernel_lights_exact_list, KF_STREAM, KB_LIGHTS | KB_EXACT | KB_LIST),
    HRT_BUILD(hrt_wgstream_kernel_views, KF_STREAM, KB_VIEWS),
    HRT_BUILD(hrt_wgstream_kernel_lights_views, KF_STREAM, KB_LIGHTS | KB_VIEWS),
    HRT_BUILD(hrt_wgstream_kernel_sph_views, KF_STREAM, KB_SPH | KB_VIEWS),
    HRT_BUILD(hrt_wgstream_kernel_lights_sph_views, KF_STREAM, KB_LIGHTS | KB_SPH | KB_VIEWS),
};

// Which build runs a launch: plain values in, a row of k_builds or an error out (in.hrt_kernel is not read: pref is its parsed
// form).  All forms give identical pixels, so this is policy; the measurements behind its thresholds are in DESIGN.md section 5.
int pick_build(const hrt_pick_input &in, KernelPref pref, const KernelBuild *&row) {
    const uint32_t flags = in.flags;
    // the streaming kernel stages the per-object tables (squares, materials, spheres, mesh records) in LDS beside its queues
    const bool stream_fits = (size_t)in.tab_rows * 16u <= 48u * 1024u;
    if ((flags & HRT_FLAG_STREAM_KERNEL) && !stream_fits)
        return fail(HRT_ERR_INVALID, "render: the scene's object tables exceed the 48 KiB the streaming kernel keeps in LDS; use another kernel form");
    const bool stream_pays = in.n_meshes > 0u || in.n_lights > 0u || (in.tiles <= 5120u && in.spp >= 8u);
    const bool stream = stream_fits && !(flags & (HRT_FLAG_WAVE_KERNEL | HRT_FLAG_DUAL_KERNEL)) &&
                        (pref.use_stream == 1 || (flags & HRT_FLAG_STREAM_KERNEL) || (pref.use_stream < 0 && stream_pays));
    const bool exact = (flags & HRT_FLAG_EXACT_ONLY) != 0u;  // proof builds exist for the lane-per-pixel and streaming forms
    if (const int rc = check_mesh_brute("render", flags)) return rc;
    if (exact && (flags & HRT_FLAG_DUAL_KERNEL)) return fail(HRT_ERR_INVALID, "render: no exact-only build of the two-stream kernel");
    const bool dual = !exact && !stream && !in.n_views && (pref.use_dual || (flags & HRT_FLAG_DUAL_KERNEL)) && in.n_meshes > 0u &&
                      !(flags & HRT_FLAG_WAVE_KERNEL);
    const KernelFamily family = stream ? KF_STREAM : (dual ? KF_DUAL : KF_LANE);
    const bool sph = stream && !exact && in.n_spheres >= HRT_SPHERE_FILTER_MIN && in.n_spheres <= 128u;  // a crowd of spheres: the pair filter
    const uint32_t bits = (in.n_lights ? KB_LIGHTS : 0u) | (exact ? KB_EXACT : 0u) | (sph ? KB_SPH : 0u) | (in.has_list ? KB_LIST : 0u) |
                          (in.n_views ? KB_VIEWS : 0u);
    for (const KernelBuild &b : k_builds)
        if (b.family == family && b.bits == bits) { row = &b; return HRT_OK; }
    return fail(HRT_ERR_INVALID, std::string("render: there is no build of the ") + (stream ? "streaming" : dual ? "two-stream" : "lane-per-pixel") + " kernel for" +
                                 (in.n_views ? " batched views" : "") + (in.has_list ? " with a tile list" : "") + (exact ? " with HRT_FLAG_EXACT_ONLY" : ""));
}

}  // namespace

struct DLensView;  // hrt_lens.hip

struct hrt_scene {
    DScene d{};                  // host copy of the device scene header
    Scratch d_scene;             // the header in HBM (read by the kernels through a constant-space pointer)
    Scratch d_cam;               // camera block in HBM, re-uploaded only when the camera changes
    Scratch d_cam_aov;           // hrt_render_aov's own camera block (it takes no part in the trace launches' ordering)
    DCamera h_cam{};
    bool cam_valid = false;
    uint32_t lds_units = 0;
    uint32_t max_leaf = 0;       // most triangles in one KD leaf (the resumable walk keeps a 16-bit leaf cursor)
    std::vector<Scratch> allocations;  // the packed arrays the header points at
    Scratch tile_counter;        // one uint32_t: the work-queue head
    Scratch stamps;              // 16 x unsigned long long: diagnostic cycle counters (HRT_STAMPS builds)
    Event ev0, ev1;              // around the last trace launch
    bool timed = false;
    float bound = 0.f;  // largest distance of any scene point from the origin (filter margins)
    // Scratch, grown on demand.  The streaming kernel's: per-workgroup samples (floats), and its path records (words) when they
    // live in global memory.  hrt_render's: the frame in tiles and in rows.  The adaptive entry points' (hrt_adaptive.hip): the
    // active tiles' sums, compact; and in ad_words the two tile lists, the judge's keep flags and the count map of
    // hrt_render_adaptive (tiles each), then the list counter.  The denoisers' (hrt_denoise.hip): the linear frame, the features,
    // the filter's scratch, the result; and for the variance-guided one the first half's sums and frame, and the variance map.
    Scratch sp_scratch, sp_pool, tiles, frame, ad_compact, ad_words, dn_frame, dn_feat, dn_scratch, dn_out, dnv_half_tiles, dnv_frame_half, dnv_var;
    uint32_t last_grid = 0, last_waves = 0, last_lds = 0;
    const KernelBuild *last_build = nullptr;  // the row of k_builds the last trace launch ran (hrt_debug_last_kernel)
    hipStream_t last_stream = nullptr;  // stream of the previous launch on this scene
    int device = 0;                     // the device that holds this scene (current when it was created)
    // hrt_render_features' own camera block, with its host copy and the launch that read it last (feature launches are ordered
    // across streams)
    Scratch d_cam_feat;
    DCamera h_cam_feat{};
    LastReader feat_reader;
    // Batched views (hrt_views.hip): the per-view blocks of the launch in hand (its last reader is the assemble launch, which also
    // read the tile sums last), the item-major tile sums of all views, and the host form's frames.
    StagedTable<DView> views;
    Scratch vw_tiles, vw_frames;
    // Batched lens views (hrt_lens.hip): the table of per-view blocks.  Nothing of the trace launches.
    StagedTable<DLensView> lens_views;
    // Adaptive lens frames (hrt_lens_adaptive.hip): the tile-major sums of the whole frame with the assemble launch that read them
    // last, and the host form's row-major frame.  The rounds' lists and keep words are ad_compact / ad_words, shared with
    // hrt_render_adaptive.  Nothing of the trace launches.
    Scratch la_tiles, la_frame;
    LastReader la_reader;
    // Light probes (hrt_probes.hip): the block values of the launch in hand, allocated by the first probe call.  Nothing of the
    // trace launches.
    Scratch pr_blocks;
    // Probe depth (hrt_probe_depth.hip): the block values of the launch in hand, allocated by the first depth call.  Nothing of
    // the trace launches.
    Scratch pd_blocks;
    // Lit probes (hrt_probe_lit.hip): the block values of the launch in hand, allocated by the first hrt_probes_lit* call.  Nothing
    // of the trace launches.
    Scratch pl_blocks;
};

namespace {

// What every entry point that works on a scene does after its own argument checks: the scene is there, the library is
// initialised, and the scene's device is current (a scene lives on its device; HIP's current device is per thread, g_rt's copy of
// it per process, so this is unconditional -- but for a call that then has nothing to do on the device: switch_device = false).
int enter_scene(const std::string &who, hrt_scene *s, bool switch_device = true) {
    if (!s) return fail(HRT_ERR_INVALID, who + ": scene is NULL");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, who + ": call hrt_init first");
    return switch_device ? use_device(s->device) : HRT_OK;
}
int enter_render(const std::string &who, hrt_scene *s, const hrt_camera *cam) {
    if (!cam) return fail(HRT_ERR_INVALID, who + ": camera is NULL");
    return enter_scene(who, s);
}

// The stats block of a render that took kernel_ms on the device and `samples` samples, started at t0.  s may be NULL for a call
// that has no scene (hrt_probe_eval).
void fill_stats(const hrt_scene *s, hrt_stats *stats, std::chrono::steady_clock::time_point t0, double kernel_ms, uint64_t samples) {
    std::memset(stats, 0, sizeof(*stats));
    stats->kernel_ms = kernel_ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    stats->samples = samples;
    stats->vgprs = (uint32_t)g_rt.attr.numRegs;
    stats->lds_bytes = s ? s->last_lds : 0u;
    stats->waves_launched = s ? s->last_waves : 0u;
}

// Uploads one packed array; the scene owns the allocation, `field` (of its header) points at it.
template <class T>
int upload_owned(hrt_scene *s, const std::vector<T> &v, const T *&field) {
    Scratch b;
    if (const int rc = b.need<T>(v.size())) return rc;
    if (const int rc = b.from_host(v.data(), v.size() * sizeof(T))) return rc;
    field = b.as<T>();
    s->allocations.push_back(std::move(b));
    return HRT_OK;
}

}  // namespace

#include "hrt_kdbuild.hip"

extern "C" {

const char *hrt_last_error(void) { return g_error.c_str(); }

int hrt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int hrt_init(int device_ordinal) {
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (n <= 0) return fail(HRT_ERR_DEVICE, "hrt_init: no HIP device");
    if (device_ordinal < 0 || device_ordinal >= n) return fail(HRT_ERR_INVALID, "hrt_init: device ordinal out of range");
    HIP_TRY(hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_ordinal));
    g_rt.device = device_ordinal;
    g_rt.cus = prop.multiProcessorCount;
    if ((int)g_rt.dev_cus.size() < n) g_rt.dev_cus.resize((size_t)n, 0);
    if (g_rt.dev_cus[device_ordinal] != 0) { g_rt.ready = true; return HRT_OK; }  // this device is prepared already: it is current again
    HIP_TRY(hipFuncGetAttributes(&g_rt.attr, (const void *)hrt_trace_kernel));
    // LDS for nodelets per 256-thread workgroup.  Default 32 KiB (4 workgroups/CU keep 128 of the
    // CU's 160 KiB); HRT_LDS_KB overrides for tuning.
    uint32_t kb = 36u * (HRT_WG / 256u);  // 4 x 36 KiB (HRT_WG 256) or 1 x 144 KiB (HRT_WG 1024) of the CU's 160 KiB
    if (const char *e = std::getenv("HRT_LDS_KB")) kb = (uint32_t)std::max(0, atoi(e));
    if (kb > 160) kb = 160;
    g_rt.lds_budget = kb * 1024u;
    // Dynamic LDS past the 64 KiB default: the lane-per-pixel builds' nodelets when the budget asks for it, the two-stream builds'
    // backed-up streams + nodelets when one big workgroup has the CU, the streaming builds' path pool (113 KiB + nodelets) always.
    const uint32_t raise[] = {g_rt.lds_budget > 64u * 1024u ? g_rt.lds_budget : 0u, HRT_WG > 256 ? 160u * 1024u : 0u, 160u * 1024u};  // by KernelFamily; 0: leave
    for (const KernelBuild &b : k_builds)
        if (raise[b.family]) HIP_TRY(hipFuncSetAttribute((const void *)b.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)raise[b.family]));
    {   // u8 -> float tables in double, as the reference evaluates c/255. and c/127.5 - 1. (Material.cpp:87,124)
        float lut[512];
        for (int c = 0; c < 256; ++c) { lut[c] = (float)(c / 255.); lut[256 + c] = (float)(c / 127.5 - 1.); }
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_u8_lut), lut, sizeof(lut)));
    }
    g_rt.pref = parse_kernel_pref(std::getenv("HRT_KERNEL"));
    g_rt.dev_cus[device_ordinal] = prop.multiProcessorCount;
    g_rt.ready = true;
    return HRT_OK;
}

void hrt_shutdown(void) { g_rt.ready = false; g_rt.dev_cus.clear(); }

void hrt_scene_destroy(hrt_scene *s) {
    if (!s) return;
    if (g_rt.ready) (void)use_device(s->device);
    delete s;  // everything it holds frees itself (the owners above)
}

// Pack on the host (hrt_pack.h: every check of the description is there), upload, then the scene's own allocations.
static int scene_create_impl(const hrt_scene_desc *desc, hrt_scene *s) {
    PackedScene P;
    std::string error;
    if (const int rc = pack_scene(*desc, P, error)) return fail(rc, error);
    DScene &d = s->d;
    d = P.header;
    s->bound = P.bound;
    s->max_leaf = P.max_leaf;
    if (const int rc = upload_owned(s, P.tabs, d.tabs)) return rc;
    if (const int rc = upload_owned(s, P.qfilter, d.qfilter)) return rc;
    if (const int rc = upload_owned(s, P.units, d.kd_units)) return rc;
    if (const int rc = upload_owned(s, P.tris, d.tris)) return rc;
    if (const int rc = upload_owned(s, P.planes, d.tri_planes)) return rc;
    if (const int rc = upload_owned(s, P.colors, d.colors)) return rc;
    if (const int rc = upload_owned(s, P.vids, d.tri_vids)) return rc;
    if (const int rc = upload_owned(s, P.images, d.images)) return rc;
    if (const int rc = upload_owned(s, P.texels, d.texels)) return rc;
    if (const int rc = upload_owned(s, P.lights, d.lights)) return rc;
    if (const int rc = upload_owned(s, P.exceptions, d.exceptions)) return rc;
    // squares | materials | spheres | mesh records live in the one array `tabs`
    d.quads = d.tabs + d.tab_quads;
    d.materials = d.tabs + d.tab_mats;
    d.spheres = d.tabs + d.tab_spheres;
    d.meshes = reinterpret_cast<const DMesh *>(d.tabs + d.tab_meshes);
    // the two things that are not the description's alone: the LDS budget and the measurement override of the pruning
    s->lds_units = std::min<uint32_t>(d.n_kd_units, g_rt.lds_budget / 16u) & ~3u;  // whole 64-byte lines: no treelet or leaf straddles
    if (const char *e = std::getenv("HRT_PRUNE")) if (e[0] == '0') d.prune_ok = 0u;  // measurement aid: the same kernels without the pruning (bench.py reports both rates)
    if (const int rc = s->tile_counter.grow(sizeof(uint32_t))) return rc;
    if (const int rc = s->stamps.grow(16 * sizeof(unsigned long long))) return rc;
    HIP_TRY(hipMemset(s->stamps.p, 0, 16 * sizeof(unsigned long long)));
    if (const int rc = s->ev0.ready()) return rc;
    if (const int rc = s->ev1.ready()) return rc;
    if (const int rc = s->d_scene.from_host(&s->d, sizeof(DScene))) return rc;
    if (const int rc = s->d_cam.grow(sizeof(DCamera))) return rc;
    return s->d_cam_aov.grow(sizeof(DCamera));
}

int hrt_scene_create(const hrt_scene_desc *desc, hrt_scene **out) {
    if (!desc || !out) return fail(HRT_ERR_INVALID, "hrt_scene_create: NULL argument");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, "hrt_scene_create: call hrt_init first");
    hrt_scene *s = nullptr;
    try {
        s = new hrt_scene();
        s->device = g_rt.device;
        int rc = scene_create_impl(desc, s);
        if (rc != HRT_OK) {
            std::string keep = g_error;
            hrt_scene_destroy(s);
            g_error = keep;
            return rc;
        }
    } catch (const std::exception &e) {
        if (s) hrt_scene_destroy(s);
        return fail(HRT_ERR_STATE, e.what());
    }
    *out = s;
    return HRT_OK;
}

uint32_t hrt_tiles_total(uint32_t w, uint32_t h) { return ((w + HRT_TILE - 1) / HRT_TILE) * ((h + HRT_TILE - 1) / HRT_TILE); }
uint32_t hrt_tiles_owned(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
    const uint32_t t = hrt_tiles_total(w, h);
    if (!world || rank >= t) return 0;
    return (t - rank + world - 1) / world;
}

// hrt_camera -> the constants camera_ray() reads (hrt_device.h DCamera).
static int make_camera(const hrt_camera *cam, DCamera &C) {
    std::memset(&C, 0, sizeof(C));
    // The GL matrices the reference reads back (matrixUtilities.h:33-46) for this pose, fp64, column-major:
    // modelview = [right; up; -forward] * translate(-eye) (Camera.cpp:125-132), projection = gluPerspective(fovy,
    // aspect, znear, zfar) (Camera.cpp:41-50) -- then inverted by the reference's own method, the adjugate over the
    // determinant term by term (matrixUtilities.h:77-206; host_invert4 above), so that every constant below carries
    // the reference's rounding.  hrt_debug_kat(HRT_KAT_CAMERA) exposes the resulting rays; tests compare them bit for
    // bit with rays produced by the reference's gluInvertMatrix + screen_space_to_world_space_ray.
    {
        double mv[16], pr[16], mi[16], pi[16];
        for (int k = 0; k < 16; ++k) { mv[k] = 0.0; pr[k] = 0.0; }
        const double Rm[3][3] = {{cam->right[0], cam->right[1], cam->right[2]},
                                 {cam->up[0], cam->up[1], cam->up[2]},
                                 {-(double)cam->forward[0], -(double)cam->forward[1], -(double)cam->forward[2]}};
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) mv[k * 4 + r] = Rm[r][k];
            mv[12 + r] = h_neg_dot3(Rm[r], cam->eye);
        }
        mv[15] = 1.0;
        const double rad = (double)cam->fovy_deg / 2.0 * M_PI / 180.0;
        const double cot = std::cos(rad) / std::sin(rad);
        const double dz = (double)cam->zfar - (double)cam->znear;
        pr[0] = cot / (double)cam->aspect;
        pr[5] = cot;
        pr[10] = -((double)cam->zfar + (double)cam->znear) / dz;
        pr[11] = -1.0;
        pr[14] = h_mul64(h_mul64(-2.0, (double)cam->znear), (double)cam->zfar) / dz;
        if (!host_invert4(mv, mi) || !host_invert4(pr, pi)) return fail(HRT_ERR_INVALID, "render: singular camera matrix");
        // The kernel evaluates the two mat-vecs of matrixUtilities.h:60-68 with their structural zeros removed, which is
        // exact only for this sparsity (a zero coefficient contributes a signed zero, and x + (+-0) == x):
        //   P^-1 = [pi0 . . .; . pi5 . .; . . . pi14; . . pi11 pi15]      MV^-1 = [* * * *; * * * *; * * * *; 0 0 0 m15]
        static const int p_zero[] = {1, 2, 3, 4, 6, 7, 8, 9, 10, 12, 13}, m_zero[] = {3, 7, 11};
        for (int k : p_zero) if (pi[k] != 0.0) return fail(HRT_ERR_INVALID, "render: projection inverse is not of the gluPerspective form");
        for (int k : m_zero) if (mi[k] != 0.0) return fail(HRT_ERR_INVALID, "render: modelview inverse is not affine");
        bool finite = true;
        for (int k = 0; k < 16; ++k) finite = finite && std::isfinite(mi[k]) && std::isfinite(pi[k]);
        if (!finite) return fail(HRT_ERR_INVALID, "render: camera is not finite");
        // resInt = P^-1 (x, y, 0, 1):  resInt0 = pi0*x, resInt1 = pi5*y, resInt2 = pi14, resInt3 = pi15   (z = GL_DEPTH_RANGE[0] = 0)
        // res_k  = ((m[k]*resInt0 + m[4+k]*resInt1) + m[8+k]*resInt2) + m[12+k]*resInt3,   res_3 = m[15]*resInt3
        const double ri2 = pi[14], ri3 = pi[15];
        for (int a = 0; a < 3; ++a) C.eye[a] = (float)(mi[12 + a] / mi[15]);  // cameraSpaceToWorldSpace(0,0,0), :53-58
        C.pi0 = pi[0]; C.pi5 = pi[5];
        C.pi15 = h_mul64(mi[15], ri3);   // res_3, the divisor of :66-68
        C.inv15 = 1.0 / C.pi15;
        for (int k = 0; k < 3; ++k) {
            C.mx[k] = mi[k];
            C.my[k] = mi[4 + k];
            C.c1[k] = h_mul64(mi[8 + k], ri2);
            C.c2[k] = h_mul64(mi[12 + k], ri3);
        }
    }
    return HRT_OK;
}

static int fill_render(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                       uint32_t flags, uint32_t rank, uint32_t world, DRender &R, DCamera &C) {
    const int frc = check_frame("render", w, h, k_max_pixels);  // the scene is the caller's to enter (enter_scene)
    if (frc != HRT_OK) return frc;
    if (!spp) return fail(HRT_ERR_INVALID, "render: spp must be positive");
    if (w > 65535u || h > 65535u) return fail(HRT_ERR_INVALID, "render: w and h must be below 65536 (tile origins are packed in 16 + 16 bits)");
    if (!world || rank >= world) return fail(HRT_ERR_INVALID, "render: bad rank/world");
    R.scene = s->d_scene.as<DScene>();
    R.lds_units = (flags & HRT_FLAG_NO_LDS_TREE) ? 0u : s->lds_units;
    R.err_abs = margin_scale(s->bound, std::sqrt(cam->eye[0] * cam->eye[0] + cam->eye[1] * cam->eye[1] + cam->eye[2] * cam->eye[2]));
    {
        const int crc = make_camera(cam, C);
        if (crc != HRT_OK) return crc;
    }
    R.w = w; R.h = h; R.spp = spp;
    R.seed_lo = (uint32_t)seed; R.seed_hi = (uint32_t)(seed >> 32);
    R.flags = flags;
    R.rank = rank; R.world = world;
    R.tiles_x = (w + HRT_TILE - 1) / HRT_TILE;
    R.tiles_total = hrt_tiles_total(w, h);
    R.tiles_owned = hrt_tiles_owned(w, h, rank, world);
    R.tile_counter = s->tile_counter.as<uint32_t>();
    R.stamps = s->stamps.as<unsigned long long>();
    R.tile_list = nullptr;
    return HRT_OK;
}

// A streaming build's launch geometry: its LDS (queues, tables, as much of the tree as fits), grid, unit and band sizes, scratch.
static int size_stream(hrt_scene *s, const KernelBuild &b, DRender &R, uint32_t &grid, uint32_t &lds_bytes) {
    const uint32_t fixed = (uint32_t)(HRT_SP_NQ * HRT_SP_POOL * 2 + HRT_SP_STREAMS * sizeof(SpCtl) + sizeof(SpShared) + HRT_SP_UNITS * sizeof(SpUnit) + HRT_SP_UNITS * HRT_SP_MAXG * 4) +
                           ((b.bits & KB_VIEWS) ? HRT_SP_UNITS * HRT_SP_MAXG * 16u : 0u) +  // the VIEWS builds' table of view rows
                           2048u + s->d.tab_rows * 16u  // + the scene's per-object tables (stream_tables_fit)
#if HRT_DIV_QUAD
                           + (s->d.n_quads + 1u) / 2u * 16u  // + the squares' side-length reciprocals, 8 bytes each (hrt_stream.hip), out of the nodelets' room
#endif
#ifdef HRT_WALK_SEG
                           + 2048u  // diagnostic build: 16 accumulators per wave
#endif
                           ;
    uint32_t per_cu = (64u * 4u * HRT_SP_MINW) / HRT_SP_WG;  // workgroups resident per CU (HRT_SP_MINW waves per SIMD in all) ...
    while (per_cu > 1u && 160u * 1024u / per_cu < fixed + 16u * 1024u) --per_cu;  // ... as far as the LDS pools allow
    const uint32_t room = (160u * 1024u / per_cu - fixed) / 16u;
    if (!(R.flags & HRT_FLAG_NO_LDS_TREE)) R.lds_units = std::min<uint32_t>(s->d.n_kd_units, room) & ~3u;  // whole 64-byte lines: no treelet or leaf straddles
    lds_bytes = fixed + R.lds_units * 16u;
    grid = std::min<uint32_t>((uint32_t)g_rt.cus * per_cu, R.tiles_owned);
    {   // tiles per work unit: as many as keep one unit (tiles x 64 pixels x samples per fold) within HRT_SP_UNIT paths
        const uint32_t per_tile = 64u * std::min<uint32_t>(R.spp, HRT_SP_SCHUNK);
        uint32_t glog = 0;
        while ((2u << glog) <= HRT_SP_MAXG && (per_tile << (glog + 1u)) <= HRT_SP_UNIT) ++glog;
        R.sp_group_log2 = glog;
        // Few, heavy tiles (a rank's share of a frame at thousands of samples per pixel): the launch ends when the last
        // workgroup finishes its last item, and an item is a whole tile's samples -- in order, so a tile cannot be split
        // across workgroups by samples.  Split it by ROWS instead: bands of 4, 2 rows until a workgroup has ~64 items.
        uint32_t band = 0;
        while (glog == 0u && band < 2u && ((uint64_t)R.tiles_owned << band) < 64ull * grid && (64u >> (band + 1u)) * (uint64_t)std::min<uint32_t>(R.spp, HRT_SP_SCHUNK) >= 4096u) ++band;
        R.sp_band_log2 = band;
    }
    int rc = s->sp_scratch.grow((size_t)grid * HRT_SP_UNITS * HRT_SP_UNIT * 3u * sizeof(float));  // HRT_SP_UNITS units in flight per workgroup
    // per workgroup the slot records, then the hit records that mirror its hit queues (1 MB, of which only [0, fill) of a queue is ever touched)
    if (rc == HRT_OK) rc = s->sp_pool.grow((size_t)grid * SP_WG_DWORDS * sizeof(uint32_t));
    if (rc != HRT_OK) return rc;
    R.sp_scratch = s->sp_scratch.as<float>();
    R.sp_pool = s->sp_pool.as<uint32_t>();
    return HRT_OK;
}

// A lane-per-pixel or two-stream build's: nodelets (and backed-up streams) in LDS, the workgroups the device keeps resident.
static int size_lanes(const KernelBuild &b, DRender &R, uint32_t &grid, uint32_t &lds_bytes) {
    const bool dual = b.family == KF_DUAL;
    lds_bytes = R.lds_units * 16u;
    if (dual) {
        // 4 workgroups per CU: 160 KiB = 4 x (27 KiB of backed-up streams + 12 KiB of nodelets)
        const uint32_t wgs = 1024u / HRT_WG, backup = HRT_DS_FIELDS * HRT_WG * 4u;
        const uint32_t room = (156u * 1024u / wgs - backup) / 16u;
        if (R.lds_units > room) R.lds_units = room & ~3u;
        lds_bytes = R.lds_units * 16u + backup;
    }
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)b.fn, HRT_WG, lds_bytes));
    if (per_cu < 1) per_cu = 1;
    grid = (uint32_t)(per_cu * g_rt.cus);
    // 4 waves per workgroup, one tile (two in the dual-stream kernel) per wave at a time
    const uint32_t per_wg = (HRT_WG / 64u) * (dual ? 2u : 1u);
    const uint32_t need = (R.tiles_owned + per_wg - 1u) / per_wg;
    if (grid > need) grid = need;
    R.sp_scratch = nullptr;
    R.sp_pool = nullptr;
    return HRT_OK;
}

// One launch of the trace kernel over this rank's tiles: samples [s0, s0 + spp) of every pixel.
struct TraceJob {
    uint32_t w, h, s0, spp;
    uint64_t seed;
    uint32_t flags;
    float *d_tiles;
    void *stream;
    uint32_t rank = 0, world = 1;
    // false: d_tiles receives the pixel means (s0 must be 0).
    // true : d_tiles holds the running sums of samples [0, s0) and receives the sums of [0, s0 + spp).
    bool accumulate = false;
    // (device, list_n rank slots; adaptive sampling): only those tiles, into a COMPACT d_tiles (entry j of the list at slot j).
    const uint32_t *list = nullptr;
    uint32_t list_n = 0;
    // != 0 (batched views, hrt_views.hip; rank 0 of world 1, no list, no accumulation): the n_views blocks staged in s->views are
    // uploaded to its device table in place of the camera block, and the queue is n_views x the frame's tiles, view-major; cam is view
    // 0's, seed is not used.  The kernel-form and grid choices see the list's tiles, or all views'.
    uint32_t n_views = 0;
};
static int launch_trace(hrt_scene *s, const hrt_camera *cam, const TraceJob &J) {
    DRender R;
    DCamera C;
    int rc = fill_render(s, cam, J.w, J.h, J.spp, J.seed, J.flags, J.rank, J.world, R, C);
    if (rc != HRT_OK) return rc;
    if (J.list) {
        if (J.list_n > R.tiles_owned) return fail(HRT_ERR_INVALID, "render: tile list longer than the rank's tiles");
        R.tile_list = J.list;
        R.tiles_owned = J.list_n;
    }
    if (J.n_views) {
        R.views = s->views.table();
        R.tiles_owned = J.n_views * R.tiles_total;
    }
    R.cam = s->d_cam.as<DCamera>();
    if (!J.d_tiles) return fail(HRT_ERR_INVALID, "render: NULL tile buffer");
    if ((uint64_t)J.s0 + J.spp > 0xffffffffull) return fail(HRT_ERR_INVALID, "render: sample index overflows 32 bits");
    R.out_tiles = J.d_tiles;
    R.s0 = J.s0;
    R.accumulate = J.accumulate ? 1u : 0u;
    const bool gamma = (J.flags & HRT_FLAG_GAMMA) && !J.accumulate;  // of sums, hrt_finalize_tiles applies the gamma
    hipStream_t stream = (hipStream_t)J.stream;
    if (R.tiles_owned == 0) { s->timed = false; return HRT_OK; }
    const KernelBuild *build = nullptr;
    const hrt_pick_input traits{s->d.n_meshes, s->d.n_lights, s->d.n_spheres, s->d.tab_rows, R.tiles_owned, J.spp, J.flags, J.list ? 1u : 0u, J.n_views, nullptr};
    if ((rc = pick_build(traits, g_rt.pref, build)) != HRT_OK) return rc;
    uint32_t grid, lds_bytes;
    rc = build->family == KF_STREAM ? size_stream(s, *build, R, grid, lds_bytes) : size_lanes(*build, R, grid, lds_bytes);
    if (rc != HRT_OK) return rc;
    s->last_grid = grid;
    s->last_lds = lds_bytes;
    s->last_waves = grid * (build->wg() / 64u);
    // One hrt_scene carries ONE launch at a time (work-queue head, stamps, path pool, camera block).  Launches on one
    // stream are ordered by the stream; a launch on another stream first waits for the previous one -- before anything of
    // its own is enqueued, the copy of a new camera block included (the previous launch may still be reading the old one).
    if (s->timed && s->last_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, s->ev1, 0));
    s->last_stream = stream;
    if (J.n_views) {
        if ((rc = s->views.upload(J.n_views, stream)) != HRT_OK) return rc;
    } else if (!s->cam_valid || std::memcmp(&C, &s->h_cam, sizeof(C)) != 0) {
        s->h_cam = C;
        HIP_TRY(hipMemcpyAsync(s->d_cam.p, &s->h_cam, sizeof(C), hipMemcpyHostToDevice, stream));
        s->cam_valid = true;
    }
    HIP_TRY(hipMemsetAsync(s->tile_counter.p, 0, sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(s->stamps.p, 0, 16 * sizeof(unsigned long long), stream));  // [15] = give-up code of the streaming kernel
    HIP_TRY(hipEventRecord(s->ev0, stream));
    hipLaunchKernelGGL(build->fn, dim3(grid), dim3(build->wg()), lds_bytes, stream, R);
    s->last_build = build;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev1, stream));
    if (gamma) {
        const uint32_t n = R.tiles_owned * 64u * 3u;
        hipLaunchKernelGGL(hrt_gamma_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, J.d_tiles, n);
        HIP_TRY(hipGetLastError());
    }
    s->timed = true;
    return HRT_OK;
}

int hrt_render_tiles(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed,
                     uint32_t flags, uint32_t rank, uint32_t world, float *d_tiles, void *stream) {
    const int rc = enter_render("hrt_render_tiles", s, cam);
    if (rc != HRT_OK) return rc;
    TraceJob job{w, h, 0u, spp, seed, flags, d_tiles, stream};
    job.rank = rank; job.world = world;
    return launch_trace(s, cam, job);
}

int hrt_render_accumulate(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t first_sample, uint32_t n_samples,
                          uint64_t seed, uint32_t flags, uint32_t rank, uint32_t world, float *d_sum_tiles, void *stream) {
    const int rc = enter_render("hrt_render_accumulate", s, cam);
    if (rc != HRT_OK) return rc;
    TraceJob job{w, h, first_sample, n_samples, seed, flags, d_sum_tiles, stream};
    job.rank = rank; job.world = world; job.accumulate = true;
    return launch_trace(s, cam, job);
}

int hrt_finalize_tiles(const float *d_sum_tiles, uint32_t n_tiles, uint32_t total_samples, uint32_t flags, float *d_tiles,
                       void *stream_) {
    if (!d_sum_tiles || !d_tiles || !total_samples) return fail(HRT_ERR_INVALID, "hrt_finalize_tiles: bad argument");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, "hrt_finalize_tiles: call hrt_init first");
    if (!n_tiles) return HRT_OK;
    const uint32_t n = n_tiles * 64u * 3u;
    hipLaunchKernelGGL(hrt_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream_, d_sum_tiles, d_tiles, n,
                       total_samples, (flags & HRT_FLAG_GAMMA) ? 1u : 0u);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

int hrt_encode_ppm(const float *d_frame, uint32_t w, uint32_t h, int format, unsigned char *d_out, size_t capacity,
                   size_t *bytes, void *stream_) {
    if (!d_frame || !d_out || !bytes || !w || !h) return fail(HRT_ERR_INVALID, "hrt_encode_ppm: bad argument");
    if (format != 3 && format != 6) return fail(HRT_ERR_INVALID, "hrt_encode_ppm: format must be 3 (ASCII) or 6 (binary)");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, "hrt_encode_ppm: call hrt_init first");
    { const int frc = check_frame("hrt_encode_ppm", w, h, k_max_records); if (frc != HRT_OK) return frc; }
    hipStream_t stream = (hipStream_t)stream_;
    char head[64];
    // main.cpp:258: "P3" endl w " " h endl 255 endl
    const int hl = std::snprintf(head, sizeof(head), "P%d\n%u %u\n255\n", format, w, h);
    const uint32_t npix = w * h;
    if (format == 6) {
        const size_t total = (size_t)hl + (size_t)npix * 3u;
        if (capacity < total) return fail(HRT_ERR_INVALID, "hrt_encode_ppm: output buffer too small (need " + std::to_string(total) + ")");
        HIP_TRY(hipMemcpyAsync(d_out, head, (size_t)hl, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(hrt_ppm6_kernel, dim3((npix * 3u + 255u) / 256u), dim3(256), 0, stream, d_frame, npix * 3u, d_out + hl);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));  // `head` is a stack buffer
        *bytes = total;
        return HRT_OK;
    }
    // P3, byte for byte what the reference's ofstream writes (main.cpp:259-261): per pixel "r g b " with each
    // value printed as a decimal int; pass 1 measures every pixel's text, a block scan turns lengths into
    // offsets, pass 2 writes the digits.  Blocks of 1024 pixels; block totals are scanned on the host side of
    // the launch (n/1024 words) to keep the device code to two simple kernels.
    const uint32_t nblocks = (npix + 1023u) / 1024u;
    Scratch len, d_base;  // every pixel's length, then the blocks' totals; the blocks' offsets
    if (const int rc = len.grow(((size_t)npix + nblocks) * sizeof(uint32_t))) return rc;
    uint32_t *const d_len = len.as<uint32_t>(), *const d_block = d_len + npix;
    hipLaunchKernelGGL(hrt_ppm3_measure_kernel, dim3(nblocks), dim3(256), 0, stream, d_frame, npix, d_len, d_block);
    std::vector<uint32_t> block(nblocks);
    HIP_TRY(hipMemcpyAsync(block.data(), d_block, nblocks * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::vector<unsigned long long> base(nblocks);
    unsigned long long run = (unsigned long long)hl;
    for (uint32_t b = 0; b < nblocks; ++b) { base[b] = run; run += block[b]; }
    const size_t total = (size_t)run + 1u;  // the closing endl
    if (capacity < total) return fail(HRT_ERR_INVALID, "hrt_encode_ppm: output buffer too small (need " + std::to_string(total) + ")");
    if (const int rc = d_base.grow(nblocks * sizeof(unsigned long long))) return rc;
    HIP_TRY(hipMemcpyAsync(d_base.p, base.data(), nblocks * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_out, head, (size_t)hl, hipMemcpyHostToDevice, stream));
    const unsigned char nl = '\n';
    HIP_TRY(hipMemcpyAsync(d_out + run, &nl, 1, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(hrt_ppm3_write_kernel, dim3(nblocks), dim3(256), 0, stream, d_frame, npix, d_len, d_base.as<unsigned long long>(), d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));  // `head`, `nl` and `base` are the call's own
    *bytes = total;
    return HRT_OK;
}

int hrt_check_last_launch(hrt_scene *s) {
    if (!s) return fail(HRT_ERR_INVALID, "hrt_check_last_launch: NULL scene");
    if (!s->timed) return HRT_OK;
    { const int drc = use_device(s->device); if (drc != HRT_OK) return drc; }
    HIP_TRY(hipEventSynchronize(s->ev1));
    unsigned long long gave_up = 0;
    HIP_TRY(hipMemcpy(&gave_up, s->stamps.as<unsigned long long>() + 15, sizeof(gave_up), hipMemcpyDeviceToHost));
    if (gave_up) return fail(HRT_ERR_DEVICE, "trace kernel gave up (scheduler cycle bound exceeded): the frame of the last launch is incomplete");
    return HRT_OK;
}

int hrt_last_kernel_ms(hrt_scene *s, double *ms) {
    if (!s || !ms) return fail(HRT_ERR_INVALID, "hrt_last_kernel_ms: NULL argument");
    if (!s->timed) { *ms = 0.0; return HRT_OK; }
    {
        const int rc = hrt_check_last_launch(s);
        if (rc != HRT_OK) return rc;
    }
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, s->ev0, s->ev1));
    *ms = (double)f;
    return HRT_OK;
}

int hrt_assemble_frame(const float *d_gathered, uint32_t tiles_per_rank_padded, uint32_t w, uint32_t h, uint32_t world,
                       float *d_frame, void *stream_) {
    if (!d_gathered || !d_frame || !w || !h || !world) return fail(HRT_ERR_INVALID, "hrt_assemble_frame: bad argument");
    if (tiles_per_rank_padded < hrt_tiles_owned(w, h, 0, world))
        return fail(HRT_ERR_INVALID, "hrt_assemble_frame: tiles_per_rank_padded too small");
    const uint32_t n = w * h;
    hipLaunchKernelGGL(hrt_assemble_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream_, d_gathered,
                       tiles_per_rank_padded, w, h, world, d_frame);
    HIP_TRY(hipGetLastError());
    return HRT_OK;
}

int hrt_debug_read_stamps(hrt_scene *s, uint64_t out[16]) {
    if (!s || !out) return fail(HRT_ERR_INVALID, "hrt_debug_read_stamps: NULL argument");
    { const int drc = use_device(s->device); if (drc != HRT_OK) return drc; }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, s->stamps.p, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return HRT_OK;
}

int hrt_debug_pick_kernel(const hrt_pick_input *in, char *name, size_t cap) {
    if (!in || !name || !cap) return fail(HRT_ERR_INVALID, "hrt_debug_pick_kernel: bad argument");
    const KernelBuild *build = nullptr;
    const int rc = pick_build(*in, parse_kernel_pref(in->hrt_kernel), build);
    std::snprintf(name, cap, "%s", build ? build->name : "");
    return rc;
}

int hrt_debug_last_kernel(hrt_scene *s, char *name, size_t cap) {
    if (!s || !name || !cap) return fail(HRT_ERR_INVALID, "hrt_debug_last_kernel: bad argument");
    std::snprintf(name, cap, "%s", s->last_build ? s->last_build->name : "");
    return HRT_OK;
}

int hrt_kernel_info(hrt_stats *out) {
    if (!out) return fail(HRT_ERR_INVALID, "hrt_kernel_info: NULL argument");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, "hrt_kernel_info: call hrt_init first");
    std::memset(out, 0, sizeof(*out));
    out->vgprs = (uint32_t)g_rt.attr.numRegs;
    out->lds_bytes = g_rt.lds_budget;
    return HRT_OK;
}

int hrt_render(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t spp, uint64_t seed, uint32_t flags,
               float *out_rgb, hrt_stats *stats) {
    if (!out_rgb) return fail(HRT_ERR_INVALID, "hrt_render: NULL output");
    int rc = enter_render("hrt_render", s, cam);  // the frame and tile buffers below belong on the scene's device
    if (rc != HRT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t tiles = hrt_tiles_total(w, h), frame_bytes = (size_t)w * h * 3 * sizeof(float);
    if ((rc = s->tiles.grow(tiles * 64 * 3 * sizeof(float))) != HRT_OK || (rc = s->frame.grow(frame_bytes)) != HRT_OK) return rc;
    rc = hrt_render_tiles(s, cam, w, h, spp, seed, flags, 0, 1, s->tiles.as<float>(), nullptr);
    if (rc != HRT_OK) return rc;
    rc = hrt_assemble_frame(s->tiles.as<float>(), (uint32_t)tiles, w, h, 1, s->frame.as<float>(), nullptr);
    if (rc != HRT_OK) return rc;
    HIP_TRY(hipMemcpy(out_rgb, s->frame.p, frame_bytes, hipMemcpyDeviceToHost));
    rc = hrt_check_last_launch(s);  // never hand back a frame the kernel did not finish
    if (rc != HRT_OK) return rc;
    if (stats) {
        double ms = 0.0;
        rc = hrt_last_kernel_ms(s, &ms);
        if (rc != HRT_OK) return rc;
        fill_stats(s, stats, t0, ms, (uint64_t)w * h * spp);
    }
    return HRT_OK;
}

int hrt_render_aov(hrt_scene *s, const hrt_camera *cam, uint32_t w, uint32_t h, uint32_t which, float *out_rgb) {
    if (!out_rgb || which > 3u) return fail(HRT_ERR_INVALID, "hrt_render_aov: bad argument");
    DRender R;
    DCamera C;
    int rc = enter_render("hrt_render_aov", s, cam);
    if (rc == HRT_OK) rc = fill_render(s, cam, w, h, 1, 0, 0, 0, 1, R, C);
    if (rc != HRT_OK) return rc;
    // A camera block of its own: a trace launch on another stream may still be reading s->d_cam.  The AOV kernel runs on the
    // null stream and hipMemcpy below waits for it, so the block is free again when this returns.
    HIP_TRY(hipMemcpy(s->d_cam_aov.p, &C, sizeof(C), hipMemcpyHostToDevice));
    R.cam = s->d_cam_aov.as<DCamera>();
    Scratch d;
    const size_t bytes = (size_t)w * h * 3 * sizeof(float);
    if ((rc = d.grow(bytes)) != HRT_OK) return rc;
    hipLaunchKernelGGL(hrt_aov_kernel, dim3((w * h + 255) / 256), dim3(256), 0, 0, R, which, d.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_rgb, d.p, bytes, hipMemcpyDeviceToHost));
    return HRT_OK;
}

int hrt_debug_path_stream(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, float *out) {
    if (!out || !n) return fail(HRT_ERR_INVALID, "hrt_debug_path_stream: bad argument");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, "hrt_debug_path_stream: call hrt_init first");
    Scratch d;
    if (const int rc = d.grow(n * sizeof(float))) return rc;
    hipLaunchKernelGGL(hrt_stream_kernel, dim3(1), dim3(64), 0, 0, (uint32_t)seed, (uint32_t)(seed >> 32), pixel, sample, n, d.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return HRT_OK;
}

void hrt_debug_live_resources(uint64_t out[4]) {
    for (int k = 0; k < 4; ++k) out[k] = g_live[k].load();
}

// Known-answer instrument: device functions on caller vectors (include/hrt.h).
int hrt_debug_kat(uint32_t which, const hrt_camera *cam, const float *prim, const float *in, uint32_t n, float *out) {
    if (!g_rt.ready) return fail(HRT_ERR_STATE, "hrt_debug_kat: call hrt_init first");
    if (!in || !out || !n) return fail(HRT_ERR_INVALID, "hrt_debug_kat: bad argument");
    static const uint32_t in_w[] = {2, 7, 7, 7, 7, 8, 3, 3, 2, 3, 7}, out_w[] = {12, 8, 2, 9, 8, 8, 3, 4, 1, 3, 8};
    if (which > HRT_KAT_QUAD_RCP) return fail(HRT_ERR_INVALID, "hrt_debug_kat: unknown instrument");
    const bool quad = which == HRT_KAT_QUAD || which == HRT_KAT_QUAD_RCP;
    if ((which == HRT_KAT_CAMERA) != (cam != nullptr) || (((which >= HRT_KAT_TRIANGLE && which <= HRT_KAT_QUAD) || quad) != (prim != nullptr)))
        return fail(HRT_ERR_INVALID, "hrt_debug_kat: cam is for HRT_KAT_CAMERA, prim for the primitive instruments");
    std::vector<float4> rows, kat_qf;
    std::vector<float> box;
    float err_abs = 0.f;
    DCamera C;
    DScene kat_scene{};   // HRT_KAT_QUAD: carries nothing but the square's filter rows
    if (which == HRT_KAT_CAMERA) {
        const int rc = make_camera(cam, C);
        if (rc != HRT_OK) return rc;
    } else if (which == HRT_KAT_TRIANGLE) {  // prim: c0, c1, c2 as handed to the Triangle constructor
        const H3 c[3] = {{prim[0], prim[1], prim[2]}, {prim[3], prim[4], prim[5]}, {prim[6], prim[7], prim[8]}};
        std::vector<float4> rest;
        fold_triangle(c, 0u, rest, rows);           // plane first, then the HRT_TRI_ROWS others (hrt_kat_triangle_kernel)
        rows.insert(rows.end(), rest.begin(), rest.end());
    } else if (which == HRT_KAT_AABB) {
        box.assign(prim, prim + 6);
    } else if (which == HRT_KAT_SPHERE) {    // prim: centre, radius, motion
        rows.push_back(make_float4(prim[0], prim[1], prim[2], prim[3]));
        rows.push_back(make_float4(prim[4], prim[5], prim[6], as_float(0u)));
    } else if (quad) {                       // prim: v0, v1, v3, motion, glass flag
        hrt_quad q;
        std::memset(&q, 0, sizeof(q));
        hrt_material m;
        std::memset(&m, 0, sizeof(m));
        for (int k = 0; k < 3; ++k) { q.v0[k] = prim[k]; q.v1[k] = prim[3 + k]; q.v3[k] = prim[6 + k]; m.motion[k] = prim[9 + k]; }
        m.type = prim[12] != 0.f ? HRT_MAT_GLASS : HRT_MAT_DIFFUSE;
        fold_quad(q, m, rows);
        build_quad_filter(rows, 1u, kat_qf, kat_scene.qf_n);
        double b = 0.0;
        for (int k = 0; k < 13; ++k) b = std::max(b, (double)std::fabs(prim[k]));
        for (size_t k = 0; k < (size_t)n * 7; ++k) if (k % 7 < 3) b = std::max(b, (double)std::fabs(in[k]));
        err_abs = margin_scale((float)(b * 4.0), 0.f);  // as fill_render derives it from the scene extent (x + 0.f is x)
    }
    Scratch prim_buf, in_buf, out_buf, qf_buf, scene_buf;
    const size_t in_bytes = (size_t)n * in_w[which] * sizeof(float), out_bytes = (size_t)n * out_w[which] * sizeof(float);
    const void *h_prim = which == HRT_KAT_CAMERA ? (const void *)&C : (which == HRT_KAT_AABB ? (const void *)box.data() : (const void *)rows.data());
    const size_t prim_bytes = which == HRT_KAT_CAMERA ? sizeof(C) : (which == HRT_KAT_AABB ? 6 * sizeof(float) : rows.size() * sizeof(float4));
    if (const int rc = prim_buf.from_host(h_prim, prim_bytes)) return rc;  // nothing where the instrument has no primitive
    if (const int rc = in_buf.from_host(in, in_bytes)) return rc;
    if (const int rc = out_buf.grow(out_bytes)) return rc;
    const void *const d_prim = prim_buf.p;
    const float *const d_in = in_buf.as<float>();
    float *const d_out = out_buf.as<float>();
    const dim3 grid((n + 255u) / 256u), block(256);
    switch (which) {
        case HRT_KAT_CAMERA: hipLaunchKernelGGL(hrt_kat_camera_kernel, grid, block, 0, 0, (const DCamera *)d_prim, d_in, n, d_out); break;
        case HRT_KAT_TRIANGLE: hipLaunchKernelGGL(hrt_kat_triangle_kernel, grid, block, 0, 0, (const float4 *)d_prim, d_in, n, d_out); break;
        case HRT_KAT_AABB: hipLaunchKernelGGL(hrt_kat_aabb_kernel, grid, block, 0, 0, (const float *)d_prim, d_in, n, d_out); break;
        case HRT_KAT_SPHERE: hipLaunchKernelGGL(hrt_kat_sphere_kernel, grid, block, 0, 0, (const float4 *)d_prim, d_in, n, d_out); break;
        case HRT_KAT_QUAD:
        case HRT_KAT_QUAD_RCP:
            if (const int rc = qf_buf.from_host(kat_qf.data(), kat_qf.size() * sizeof(float4))) return rc;
            kat_scene.qfilter = qf_buf.as<float4>();
            if (const int rc = scene_buf.from_host(&kat_scene, sizeof(DScene))) return rc;
            if (which == HRT_KAT_QUAD) hipLaunchKernelGGL(hrt_kat_quad_kernel, grid, block, 0, 0, (const float4 *)d_prim, scene_buf.as<const DScene>(), d_in, n, err_abs, d_out);
            else hipLaunchKernelGGL(hrt_kat_quad_rcp_kernel, grid, block, 0, 0, (const float4 *)d_prim, scene_buf.as<const DScene>(), d_in, n, err_abs, d_out);
            break;
        case HRT_KAT_OPTICS: hipLaunchKernelGGL(hrt_kat_optics_kernel, grid, block, 0, 0, d_in, n, d_out); break;
        case HRT_KAT_HITWORD: hipLaunchKernelGGL(hrt_kat_hitword_kernel, grid, block, 0, 0, d_in, n, d_out); break;
        case HRT_KAT_DIV_KNOWN: hipLaunchKernelGGL(hrt_kat_div_known_kernel, grid, block, 0, 0, d_in, n, d_out); break;
        case HRT_KAT_NORMALIZE_SHARED: hipLaunchKernelGGL(hrt_kat_normalize_shared_kernel, grid, block, 0, 0, d_in, n, d_out); break;
        default: hipLaunchKernelGGL(hrt_kat_normalize_kernel, grid, block, 0, 0, d_in, n, d_out); break;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
    return HRT_OK;
}

// main.cpp:252-262: "P3", one line of "(int)(255*min(1,c))" triples.
int hrt_write_ppm(const char *path, const float *rgb, uint32_t w, uint32_t h) {
    if (!path || !rgb) return fail(HRT_ERR_INVALID, "hrt_write_ppm: NULL argument");
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(HRT_ERR_IO, std::string("Could not open file: ") + path);
    std::fprintf(f, "P3\n%u %u\n255\n", w, h);
    const size_t n = (size_t)w * h;
    for (size_t i = 0; i < n; ++i) {
        int c[3];
        for (int k = 0; k < 3; ++k) c[k] = (int)(255.f * std::min<float>(1.f, rgb[3 * i + k]));
        std::fprintf(f, "%d %d %d ", c[0], c[1], c[2]);
    }
    std::fprintf(f, "\n");
    std::fclose(f);
    return HRT_OK;
}

#include "hrt_multi.hip"
#include "hrt_adaptive.hip"
#include "hrt_denoise.hip"
#include "hrt_temporal.hip"
#include "hrt_rays.hip"
#include "hrt_radiance.hip"
#include "hrt_lens.hip"
#include "hrt_bake.hip"
#include "hrt_probes.hip"
#include "hrt_probe_depth.hip"
#include "hrt_probe_volume.hip"
#include "hrt_probe_lit.hip"
#include "hrt_lit_paths.hip"
#include "hrt_path_features.hip"
#include "hrt_lit_frames.hip"
#include "hrt_bake_lit.hip"
#include "hrt_lens_adaptive.hip"
#include "hrt_lit_adaptive.hip"
#include "hrt_views.hip"

int hrt_kd_build_gpu(const hrt_kd_build_input *in, hrt_kd_build_output *out, void *user) {
    (void)user;
    if (!in || !out || (in->n_refs && (!in->ids || !in->lo || !in->hi))) return fail(HRT_ERR_INVALID, "hrt_kd_build_gpu: bad argument");
    if (!g_rt.ready) return fail(HRT_ERR_STATE, "hrt_kd_build_gpu: call hrt_init first");
    std::memset(out, 0, sizeof(*out));
    {
        const int drc = use_device(g_rt.device);
        if (drc != HRT_OK) return drc;
    }
    try {
        return kd_build_gpu_impl(in, out);
    } catch (const std::exception &e) {
        return fail(HRT_ERR_STATE, std::string("hrt_kd_build_gpu: ") + e.what());
    }
}

}  // extern "C"
