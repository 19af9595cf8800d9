// avr_capi.hip — host side of libavr_hip.so: the C-ABI (include/avr.h) and the
// wavefront scheduler that replaces pbrt's ImageTileIntegrator::Render /
// WavefrontPathIntegrator::Render loops (cpu/integrators.cpp:72-232,
// wavefront/integrator.cpp:290-493) for the volumetric path.
//
// Scheduling: the requested sample range is cut into passes of S sample indices
// over all P pixels (P*S <= max_paths, default 16M paths in flight for the wavefront
// kernels and 64M 32-B sample records for k_paths — HBM is 288 GB, pbrt's GPU path caps at 1M). Each pass: k_camera, then depth iterations of
// {k_medium, k_shadow} over compacted queues until no path survives, then k_film.
// Everything is enqueued on one HIP stream; the host reads back one int (the
// survivor count) per depth iteration to size the next launch and stop early.
#include "avr_kernels.hip"
#include "avr_kpaths_list.h"
#include "avr_kpaths_slot.h"
#ifdef AVR_KP_SPLIT
// k_paths is instantiated in avr_kpaths.hip's translation units (one per medium kind and
// render mode, compiled in parallel by build.py); declared here, launched from avr_render
namespace avr {
#define AVR_KP_DECL(em, gr, zs, med, im, fa) extern template __global__ void k_paths<em, gr, zs, med, im, fa>(Params);
AVR_KP_ALL(AVR_KP_DECL)
#undef AVR_KP_DECL
}  // namespace avr
#endif
#include "avr_graph.hip"
#include "avr_devmem.h"
#include "../../include/avr.h"

#include <rccl/rccl.h>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(AVR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
    } while (0)

}  // namespace

using avr::devmem::Arena;
using avr::devmem::Buffer;

// The camera set: k_paths' per-sample records, its camera stage's buffers (PathSoA's rec, cam0..5,
// camw) and the work heads the stage resets. The one place that lists them.
struct CameraSet {
    Buffer<float4> rec, cam0, cam1, cam2, cam4;
    Buffer<uint4> cam3, cam5;
    Buffer<float> camw;
    Buffer<int> heads;   // 8 per-XCD work counters of k_paths + the pass generation
    template <typename F>
    void each_buffer(F f) { f(rec); f(cam0); f(cam1); f(cam2); f(cam3); f(cam4); f(cam5); f(camw); }
    // point a launch's arguments at this set
    void point(avr::Params &p) const {
        p.ps.rec = rec.get(); p.ps.camw = camw.get(); p.heads = heads.get();
        p.ps.cam0 = cam0.get(); p.ps.cam1 = cam1.get(); p.ps.cam2 = cam2.get(); p.ps.cam3 = cam3.get();
        p.ps.cam4 = cam4.get(); p.ps.cam5 = cam5.get();
    }
    // the eight per-sample buffers for n samples (on failure, those allocated stay for free_buffers;
    // each_buffer visits every one, so the chain is what stops at the first failure)
    hipError_t alloc_buffers(size_t n) {
        hipError_t e = hipSuccess;
        each_buffer([&](auto &b) { if (e == hipSuccess) e = b.alloc(n); });
        return e;
    }
    // heads that no pass generation matches
    hipError_t alloc_heads() {
        const hipError_t e = heads.alloc(9);
        return e == hipSuccess ? hipMemset(heads.get(), 0xff, 9 * sizeof(int)) : e;
    }
    void free_buffers() { each_buffer([](auto &b) { b.reset(); }); }
    void free_heads() { heads.reset(); }
};

// The wavefront kernels' path state (PathSoA, ShadowSoA) and queues, one buffer per array
struct PathBuffers {
    Buffer<float4> o, d, lambda, pdf, beta, r_u, r_l, L, sh_o, sh_d, sh_bf, sh_Ls, sh_rp;
    Buffer<uint64_t> smp_state, smp_inc;
    Buffer<int> depth, sh_path, queue[2];
    Buffer<float> weight;
    Buffer<float2> sh_pdfs;
    template <typename F>
    void each_buffer(F f) {
        f(o); f(d); f(lambda); f(pdf); f(beta); f(r_u); f(r_l); f(L); f(smp_state); f(smp_inc); f(depth); f(weight);
        f(sh_path); f(sh_o); f(sh_d); f(sh_bf); f(sh_Ls); f(sh_rp); f(sh_pdfs); f(queue[0]); f(queue[1]);
    }
    // the kernels' views (the k_paths records and camera stage are not in them: CameraSet)
    void point(avr::PathSoA &ps, avr::ShadowSoA &sh) const {
        ps = {};
        ps.o = o.get(); ps.d = d.get(); ps.lambda = lambda.get(); ps.pdf = pdf.get(); ps.beta = beta.get();
        ps.r_u = r_u.get(); ps.r_l = r_l.get(); ps.L = L.get(); ps.smp_state = smp_state.get();
        ps.smp_inc = smp_inc.get(); ps.depth = depth.get(); ps.weight = weight.get();
        sh = {sh_path.get(), sh_o.get(), sh_d.get(), sh_bf.get(), sh_Ls.get(), sh_rp.get(), sh_pdfs.get()};
    }
};

constexpr int kPtabKey = 8;   // what a built ZSobol pass table depends on (ptab_key)

// Pass overlap: k_paths is held to four blocks per CU while a camera stage runs beside it
// (pass_kpaths, avr_render.hip); the dynamic LDS that keeps a fifth block off a CU: 4 x (k_paths'
// 31.5 KB + pad) + the camera block's 28.3 KB fit the 160 KiB, 5 x (31.5 KB + pad) do not
// (tests/test_overlap_resources.py reads the value from this file)
constexpr int kOverlapLdsPad = 1536;

// What the side stream holds (or is making) for the pass expected next: its ZSobol pass table
// (avr_set_pass_table_ahead) and, with pass overlap, its camera records in the other camera set.
struct LookAhead {
    bool tab_valid = false;   // a table for `key` in pass-table buffer `buf`
    long long key[kPtabKey] = {};
    int buf = 0;
    bool cam_valid = false;   // ... and camera records made with the arguments `params`, at setup generation `gen`
    avr::Params params{};
    unsigned long long gen = 0;
    void invalidate() { tab_valid = cam_valid = false; }
    // Take what was built ahead for the pass that `k` names. `stream` waits for the side stream's
    // work (ev_tab) whether it is used or not, so no build of this pass overlaps it. *b: the
    // table's buffer, or -1 when none was built for this pass; *cam: camera records came with it
    // and no setup call or readback (cfg_gen) came between. Nothing stays claimed.
    hipError_t claim(hipStream_t stream, hipEvent_t ev_tab, const long long *k, unsigned long long cfg_gen, int *b,
                     bool *cam) {
        *b = -1;
        *cam = false;
        if (!tab_valid) return hipSuccess;
        const hipError_t e = hipStreamWaitEvent(stream, ev_tab, 0);
        if (e != hipSuccess) return e;
        const bool same = std::equal(k, k + kPtabKey, key);
        if (same) *b = buf;
        *cam = same && cam_valid && gen == cfg_gen;
        invalidate();
        return hipSuccess;
    }
    void publish(const long long *k, int b, const avr::Params *cam_params, unsigned long long cfg_gen) {
        std::copy(k, k + kPtabKey, key);
        buf = b;
        tab_valid = true;
        cam_valid = cam_params != nullptr;
        if (cam_params) params = *cam_params, gen = cfg_gen;
    }
};

// The last pass rendered, written once per pass by the integrator that ran it and read by the
// avr_last_*, avr_graph_last_pass and avr_graph_analyze_last_pass readbacks
struct LastPass {
    bool persistent = false;   // k_paths (else the wavefront kernels or a graph integrator)
    bool fast = false;         // ... in fast mode
    bool graph = false;        // avr_graph_render's or avr_graph_render_uniform's
    int analyze = 0;           // avr_graph_analyze's: 1 without, 2 with detail
    int analyze_depth = 0;     // ... and its max_depth (the detail's stride)
    int base = 0, S = 0;       // sample indices [base, base + S)
    int order_gen = 0;         // the pixel-order generation its k_paths records are in
    // of the last k_paths pass (a pass of another integrator carries them over): it took camera
    // records made ahead (avr_pass_overlap_active); its slot in the kernel table, -1 none yet
    // (avr_last_kernel, so a profiler pass can be matched to the timed run)
    bool overlap = false;
    int variant = -1;
    // the record of a pass [base, base + S) that ran other kernels than k_paths
    LastPass without_kpaths(int b, int s) const {
        LastPass n;
        n.base = b; n.S = s; n.overlap = overlap; n.variant = variant;
        return n;
    }
};

struct avr_context {
    int device = 0;
    // paths per pass: max_paths when the caller set one, else 16M for the wavefront kernels
    // (full SoA path state, ~250 B per path) and 64M for k_paths (a 32-B record per sample
    // only: 2 GiB of HBM; longer passes amortise the persistent kernel's drain tail)
    long long max_paths = 16ll << 20;
    bool max_paths_set = false;
    long long rec_cap = 0;   // k_paths records and camera stage allocated (samples)
    // The streams and events come before every device buffer: members go in reverse order, so the
    // buffers are freed (avr_context_destroy: on the context's device, both streams drained)
    // before the streams are destroyed. tstream, ev_cam, ev_tab: the side stream (LookAhead).
    avr::devmem::Stream own_stream, tstream;
    hipStream_t stream = nullptr;
    avr::devmem::Event ev_cam, ev_tab;
    std::vector<avr::devmem::Event> evpool;   // timing events; the first ev_used are recorded, unresolved
    // medium
    avr::DevMedium med{};
    Buffer<float> d_density_owned;
    Buffer<float> d_sigma_a, d_sigma_s, d_Le, d_lescale, d_majorant;
    bool has_medium = false;
    // lights / camera / film
    avr::DevLights lights{};
    Buffer<float> d_lightL;
    Buffer<avr::DevLight> d_lights;
    avr::DevCamera cam{};
    bool has_camera = false;
    avr::DevFilm film{};   // its sums: d_film_rgb, d_film_w, d_film_bucket ({bucket_sum, bucket_w})
    Buffer<double> d_film_rgb, d_film_w, d_film_bucket;
    Buffer<float> d_xyz;
    bool has_film = false;
    // path state
    long long cap = 0;
    avr::PathSoA ps{};
    avr::ShadowSoA sh{};
    PathBuffers paths;
    Buffer<int> d_counts;  // [0],[1] queue counts, [2] shadow count
    Buffer<unsigned long long> d_stats;
    avr::devmem::PinnedInts h_count;
    avr_stats stats{};
    size_t ev_used = 0;
    struct Timed { int a, b; double avr_stats::*field; bool launch; };
    std::vector<Timed> timed;         // pending (event a -> event b) intervals to fold into stats
    LastPass last;
    int kernel_mode = 0;      // 0: persistent k_paths (default), 1: wavefront k_medium/k_shadow
    int pass_gen = 0;         // k_paths passes enqueued (the camera stage stamps it into its set's heads[8])
    // k_paths' pixel order (avr_set_pixel_order): slot -> pixel and pixel -> slot, and the
    // host copy of the latter (to return the last pass in pixel order); empty = scanline
    Buffer<int> d_pix_order, d_pix_slot;
    std::vector<int> h_pix_slot;
    // bumped whenever the pixel order changes (avr_set_pixel_order, avr_film); the last
    // render's records are in the order of generation last.order_gen
    int order_gen = 0;
    // the k_paths instantiations by slot (avr_kpaths_slot.h), each one's persistent grid and name
    static constexpr int kNumPaths = avr::kp::kNumSlots;
    int paths_grid[kNumPaths] = {};
    void (*kpaths[kNumPaths])(avr::Params) = {};
    const char *kpaths_name[kNumPaths] = {};
    int render_mode = 0;      // 0 replay (canonical math, per-sample parity), 1 fast (hardware math)
    int ray_binning = 0;      // wavefront organisation: counting-sort queues by (majorant cell, octant)
    int majorant_occupancy = 0;   // NanoVDB k_paths: coarse occupancy level of the majorant in LDS (opt-in)
    Buffer<unsigned> d_occ;
    Buffer<float4> d_planes;   // convex interface half-spaces (avr_medium_boundary_convex)
    Buffer<int> d_bin_keys, d_bin_out, d_bin_hist;
    // pixel sampler (avr_set_sampler) and filter (avr_set_filter)
    int sampler_kind = 0;     // 0 IndependentSampler, 1 ZSobolSampler
    int sampler_spp = 16;     // samplesPerPixel of the sampler (ZSobol's Morton layout)
    int filter_type = 0;      // 0 BoxFilter (radius from avr_film), 1 GaussianFilter
    Buffer<float> d_filter;
    Buffer<float> d_temperature;
    // NanoVDBMedium grids (0 density, 1 temperature): block slots, leaves, tile values
    Buffer<int> d_vdb_slot[2];
    Buffer<float> d_vdb_leaves[2], d_vdb_tiles[2];
    int vdb_ibbox[6] = {};    // density grid's active index bbox (majorant clamp)
    long long vdb_napron[2] = {0, 0};   // apron blocks of the density / temperature grid
    // RGBGridMedium grids (sigma_a, sigma_s, Le as float4 {c0, c1, c2, scale}) and illuminant
    Buffer<float4> d_rgb[3];   // owned copies (avr_medium_rgbgrid only)
    Buffer<float> d_illum;
    // lights: host copy of the device list, ImageInfiniteLight buffers
    avr::DevLight h_lights[avr::kMaxLights] = {};
    // PowerLightSampler: each light's Phi-based weight (phi_ok once known: an image light's
    // needs its avr_light_image), and the sampler the render uses (0 BVH / uniform, 1 power)
    float h_phi[avr::kMaxLights] = {};
    bool phi_ok[avr::kMaxLights] = {};
    int light_sampler = 0;
    Buffer<unsigned char> d_light_img[avr::kMaxLights];
    int n_image_lights = 0;
    // PointLight / SpotLight: how many the list holds, which have their avr_light_local, their
    // renderFromLight (4x4; the device record keeps the position and lightFromRender's 3x3), the
    // host copy of the lights' tables (Phi and the bounds' I->MaxValue()) and the light BVH
    int n_local_lights = 0;
    bool local_ok[avr::kMaxLights] = {};
    float h_rfl[avr::kMaxLights][16] = {};
    std::vector<float> h_lightL;
    avr::ll::Tree h_tree{};
    // film image / --mse-reference-image state
    Buffer<float> d_image, d_reference;
    Buffer<double> d_metric;      // kMetricBlocks * kMetricSlots partials + kMetricSlots totals
    avr::Mat3 ref_out_from_sensor{};
    int ref_fp16 = 1;
    avr::smp::FilterTables ftab{};
    // ZSobol pixel table (zsobol_upper per Morton(pixel) x dimension < zs_dims), rebuilt
    // when the sampler's spp or the film resolution change; zs_dims 0 = no table
    Buffer<uint32_t> d_zs_table;
    int zs_dims = 256;
    int zs_key[3] = {-1, -1, -1};
    // ZSobol pass table (zsobol_pass_entry per Morton(pixel) x dimension < zs_pdims), rebuilt
    // for every k_paths pass: the digits its sample indices share; zs_pdims 0 = no table
    // Two buffers: a pass reads one while the next pass's table is built ahead into the other
    // (ptab_spec) on the low-priority side stream tstream
    Buffer<uint64_t> d_zs_ptab[2];
    Buffer<uint64_t> d_zs_ctab[2];  // the camera stage's compact copy (6 entries per pixel)
    int zs_pdims = 96;
    int tab_buf = 1;              // the buffer the last pass read
    int ptab_spec = 1;            // avr_set_pass_table_ahead
    LookAhead look;               // what tstream holds (or is building) for the next pass
    long long prev_call_begin = -1;   // avr_render's previous spp_begin (the call stride)
    // Pass overlap (avr_set_pass_overlap): behind the table built ahead, tstream also runs the
    // next pass's camera stage, into the other camera set (alt; set always names the set of the
    // last rendered pass), while this pass's k_paths runs. The pass that follows takes those
    // records when its camera stage's kernel arguments equal look.params byte for byte and no
    // setup call or readback came between (cfg_gen, bumped by AVR_QUIESCE); otherwise it runs
    // its own camera stage.
    int pass_overlap = 1;
    int num_cus = 0;
    CameraSet set, alt;               // set.heads lives as long as the context, the rest by ensure_records / ensure_alt
    long long alt_cap = 0;            // samples the other set holds (rec_cap, or 0: none)
    long long alt_failed_cap = 0;     // the rec_cap at which its allocation failed (not retried)
    unsigned long long cfg_gen = 0;
    // Level-A pass table (the same table for plo + 2, shared by four consecutive passes);
    // zs_akey names the build it holds (rebuilt when any field changes)
    Buffer<uint64_t> d_zs_atab;
    long long zs_akey[6] = {-1, -1, -1, -1, -1, -1};
    int refill_min = 0;       // 0: the default (32 lanes; 20 for a non-emissive NanoVDB walk, 16 for RGB grids, 48 for a <= 2^3 GridMedium majorant)
    int refill_batch = 0;     // 0: the default of the medium kind (walk_schedule)
    int dda_budget = 0;       // 0: by majorant resolution (12 cells up to 16^3, 32 for NanoVDB's 64^3)
    int grid_layout = 1;
    bool gray = false;        // sigma_a and sigma_s constant over 360..830 nm      // 1: build the fat (footprint) copy when memory allows, 0: linear only
    Buffer<float4> d_fat;
    Buffer<float> d_brick;   // bricked GridMedium copy (grid_layout 2)
    Buffer<uint64_t> d_advance;  // per-pass PCG advance table {A, H}
    // avr_film_reduce_rccl: this context's communicator and the clique (contexts in rank
    // order) it was created with by ncclCommInitAll; reused while the same clique reduces
    ncclComm_t comm = nullptr;
    std::vector<avr_context *> comm_group;
    // graph render (avr_graph_render / avr_graph_connect): the device copy of the last index
    // used, named by the index's id (an address could be reused by a later index); one
    // allocation behind gidx's pointers. d_gside: the pass's {scatter point, neighbour count}.
    unsigned long long gidx_uid = 0;
    Buffer<char> d_gidx;
    avr::graph::IndexView gidx{};
    Buffer<float4> d_gside;
    // the uniform graph's table (avr_graph_render_uniform, avr_graph_uniform_*_device): the device
    // copy of the last one used, under the graph's id as gidx is
    unsigned long long guni_uid = 0;
    Buffer<avr::graph::UniformEntry> d_guni;
    avr::graph::UniformView guni{};
    // the graph tools' primitive (avr_graph_set_geometry): 0 the bounds box, 1 the interface
    int graph_geometry = 0;
    // graph analysis (avr_graph_analyze): the pass's per-sample records, the per-pixel sums
    // (made by the first analysis on a film, dropped with the film) and, only when a call asks
    // for it, the pass's per-scatter detail
    Buffer<avr::graph::AnalyzeRec> d_arec;
    Buffer<avr::graph::AnalyzeAcc> d_aacc;
    Buffer<avr::graph::AnalyzeDetail> d_adetail;
};

namespace {

// Destroy the communicators of c's RCCL clique (every member's: a clique with one member
// gone cannot run a collective) and forget the clique on each member.
void release_comms(avr_context *c) {
    if (!c || c->comm_group.empty()) return;
    const std::vector<avr_context *> group = c->comm_group;
    for (avr_context *m : group) {
        if (m->comm) {
            (void)hipSetDevice(m->device);
            (void)ncclCommDestroy(m->comm);
        }
        m->comm = nullptr;
        m->comm_group.clear();
    }
    (void)hipSetDevice(c->device);
}

void free_paths(avr_context *c) {
    c->paths.each_buffer([](auto &b) { b.reset(); });
    // (the k_paths records and camera stage are not in ps: c->set, managed by ensure_records)
    c->ps = {};
    c->sh = {};
    c->cap = 0;
}

void free_pixel_order(avr_context *c) {
    if (c->d_pix_order) ++c->order_gen;   // back to scanline order
    c->d_pix_order.reset();
    c->d_pix_slot.reset();
    c->h_pix_slot.clear();
}

// The other set of records, camera buffers and work heads (pass overlap)
void free_alt(avr_context *c) {
    c->alt.free_buffers();
    c->alt.free_heads();
    c->alt_cap = 0;
}

void free_records(avr_context *c) {
    // camera records made ahead may still be written: let the side stream finish, and drop them
    if (c->tstream && c->alt_cap) (void)hipStreamSynchronize(c->tstream);
    c->look.cam_valid = false;
    c->set.free_buffers();
    c->rec_cap = 0;
    free_alt(c);
}

// The film's sums (they go with the film, its pixel bounds or, the bucket sums, its buckets)
void free_film_sums(avr_context *c) {
    c->d_film_rgb.reset();
    c->d_film_w.reset();
    c->d_film_bucket.reset();
    c->film.rgb_sum = c->film.w_sum = c->film.bucket_sum = c->film.bucket_w = nullptr;
}

// ... for the film's bounds and buckets
int alloc_film_sums(avr_context *c) {
    const size_t np = (size_t)c->film.bw * c->film.bh;
    if (!c->d_film_rgb) {
        HIP_TRY(c->d_film_rgb.alloc(3 * np));
        HIP_TRY(c->d_film_w.alloc(np));
        c->film.rgb_sum = c->d_film_rgb.get();
        c->film.w_sum = c->d_film_w.get();
    }
    if (c->film.nbuckets > 0) {
        const size_t nb = np * c->film.nbuckets;
        HIP_TRY(c->d_film_bucket.alloc(2 * nb));
        c->film.bucket_sum = c->d_film_bucket.get();
        c->film.bucket_w = c->film.bucket_sum + nb;
    }
    return AVR_OK;
}

// ... as large as the first set. Without room for it the passes keep the serial chain (no error).
void ensure_alt(avr_context *c) {
    if (c->alt_cap == c->rec_cap || c->alt_failed_cap == c->rec_cap) return;
    if (c->alt.alloc_buffers((size_t)c->rec_cap) == hipSuccess && c->alt.alloc_heads() == hipSuccess) {
        c->alt_cap = c->rec_cap;
        return;
    }
    (void)hipGetLastError();
    free_alt(c);
    c->alt_failed_cap = c->rec_cap;
}

// k_paths' per-sample records (L, 16 B) and its camera stage (k_paths_camera: 6 x 16 B + the
// 4-B filter weight), independent of the wavefront SoA
int ensure_records(avr_context *c, long long n) {
    if (n <= c->rec_cap) return AVR_OK;
    free_records(c);
    HIP_TRY(c->set.alloc_buffers((size_t)n));
    c->rec_cap = n;
    return AVR_OK;
}

int ensure_paths(avr_context *c, long long n) {
    if (n <= c->cap) return AVR_OK;
    free_paths(c);
    hipError_t e = hipSuccess;   // (each_buffer visits every array: the chain stops at the first failure)
    c->paths.each_buffer([&](auto &b) { if (e == hipSuccess) e = b.alloc((size_t)n); });
    HIP_TRY(e);
    c->paths.point(c->ps, c->sh);
    c->cap = n;
    return AVR_OK;
}

void copy_xf(avr::Xf &x, const float m[16]) {
    for (int i = 0; i < 12; ++i) x.m[i] = m[i];
}

int upload_table(Buffer<float> &dst, const float *src, size_t n, hipStream_t s) {
    dst.reset();
    if (!src) return AVR_OK;
    HIP_TRY(dst.alloc(n));
    HIP_TRY(hipMemcpyAsync(dst.get(), src, n * sizeof(float), hipMemcpyHostToDevice, s));
    return AVR_OK;
}

int blocks_for(long long n, int per = 256, int cap = 256 * 16) {
    long long b = (n + per - 1) / per;
    if (b < 1) b = 1;
    return (int)std::min<long long>(b, cap);
}

bool affine(const float m[16]) { return m[12] == 0 && m[13] == 0 && m[14] == 0 && m[15] == 1; }

void free_rgb(avr_context *c) {
    for (auto &b : c->d_rgb) b.reset();
    c->d_illum.reset();
    c->med.rgb_a = c->med.rgb_s = c->med.rgb_le = nullptr;
    c->med.illuminant = nullptr;
}

void free_vdb(avr_context *c) {
    for (int k = 0; k < 2; ++k) {
        c->d_vdb_slot[k].reset();
        c->d_vdb_leaves[k].reset();
        c->d_vdb_tiles[k].reset();
    }
    c->med.vdb = {};
    c->med.vdb_temp = {};
}

// Map::set (NanoVDB): the float inverse matrix and translation are roundings of the f64 map
template <typename GridT>
bool vdb_map(const avr_vdb_grid *G, GridT &g) {
    for (int k = 0; k < 9; ++k) {
        if (!std::isfinite(G->world_to_index[k])) return false;
        g.inv[k] = (float)G->world_to_index[k];
    }
    for (int r = 0; r < 3; ++r) g.vec[r] = (float)G->index_to_world[4 * r + 3];
    return true;
}

// GridData::mWorldBBox: the map (Map::applyMap, f64) of the 8 corners of [min, max + 1]
void vdb_world_bbox(const avr_vdb_grid *G, double lo[3], double hi[3]) {
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    const double *M = G->index_to_world;
    for (int corner = 0; corner < 8; ++corner) {
        const double x = (corner & 1) ? G->index_bbox[3] + 1.0 : G->index_bbox[0];
        const double y = (corner & 2) ? G->index_bbox[4] + 1.0 : G->index_bbox[1];
        const double z = (corner & 4) ? G->index_bbox[5] + 1.0 : G->index_bbox[2];
        for (int r = 0; r < 3; ++r) {
            const double w = M[4 * r] * x + M[4 * r + 1] * y + M[4 * r + 2] * z + M[4 * r + 3];
            lo[r] = std::min(lo[r], w);
            hi[r] = std::max(hi[r], w);
        }
    }
}

// Flatten one tree into the block-slot layout of avr_vdb.h, then into its apron layout on
// the device (what the kernels sample)
int upload_vdb(avr_context *c, const avr_vdb_grid *G, int k, avr::vdb::Apron &g) {
    if (G->n_leaves < 0 || G->n_tiles < 0 || (G->n_leaves && (!G->leaf_origin || !G->leaf_values)) ||
        (G->n_tiles && (!G->tile_origin || !G->tile_size || !G->tile_value)))
        return fail(AVR_ERR_ARG, "bad vdb grid arrays");
    for (int a = 0; a < 3; ++a)
        if (G->index_bbox[a] > G->index_bbox[3 + a]) return fail(AVR_ERR_ARG, "empty vdb index bbox");
    g = {};
    if (!vdb_map(G, g)) return fail(AVR_ERR_ARG, "non-finite vdb world-to-index map");
    g.background = G->background;
    long long lo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, hi[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN};
    auto extend = [&](const int *o, long long size) {
        for (int a = 0; a < 3; ++a) { lo[a] = std::min<long long>(lo[a], o[a]); hi[a] = std::max<long long>(hi[a], o[a] + size); }
    };
    for (int l = 0; l < G->n_leaves; ++l) {
        const int *o = G->leaf_origin + 3 * l;
        if ((o[0] & 7) || (o[1] & 7) || (o[2] & 7)) return fail(AVR_ERR_ARG, "leaf origin not a multiple of 8");
        extend(o, 8);
    }
    for (int t = 0; t < G->n_tiles; ++t) {
        const int *o = G->tile_origin + 3 * t;
        const int sz = G->tile_size[t];
        if (sz < 8 || (sz & 7) || (o[0] & 7) || (o[1] & 7) || (o[2] & 7))
            return fail(AVR_ERR_ARG, "tile origin/size not multiples of 8");
        extend(o, sz);
    }
    long long nb[3] = {0, 0, 0};
    if (G->n_leaves + G->n_tiles > 0)
        for (int a = 0; a < 3; ++a) nb[a] = (hi[a] - lo[a]) / 8;
    const long long nslot = nb[0] * nb[1] * nb[2];
    if (nslot > (1ll << 31)) return fail(AVR_ERR_ARG, "vdb grid extent too large (> 2^31 blocks)");
    std::vector<int> slot((size_t)std::max<long long>(nslot, 1), avr::vdb::kBackgroundSlot);
    auto sidx = [&](long long bx, long long by, long long bz) { return (size_t)((bz * nb[1] + by) * nb[0] + bx); };
    for (int t = 0; t < G->n_tiles; ++t) {
        const int *o = G->tile_origin + 3 * t;
        const long long s = G->tile_size[t] / 8;
        const long long bx0 = (o[0] - lo[0]) / 8, by0 = (o[1] - lo[1]) / 8, bz0 = (o[2] - lo[2]) / 8;
        for (long long bz = bz0; bz < bz0 + s; ++bz)
            for (long long by = by0; by < by0 + s; ++by)
                for (long long bx = bx0; bx < bx0 + s; ++bx) slot[sidx(bx, by, bz)] = -(t + 1);
    }
    for (int l = 0; l < G->n_leaves; ++l) {
        const int *o = G->leaf_origin + 3 * l;
        int &s = slot[sidx((o[0] - lo[0]) / 8, (o[1] - lo[1]) / 8, (o[2] - lo[2]) / 8)];
        if (s >= 0) return fail(AVR_ERR_ARG, "duplicate leaf origin");
        s = l;
    }
    avr::vdb::Grid base{};
    base.background = g.background;
    for (int q = 0; q < 9; ++q) base.inv[q] = g.inv[q];
    for (int q = 0; q < 3; ++q) base.vec[q] = g.vec[q];
    base.ox = nslot ? (int)lo[0] : 0; base.oy = nslot ? (int)lo[1] : 0; base.oz = nslot ? (int)lo[2] : 0;
    base.lnx = (int)nb[0]; base.lny = (int)nb[1]; base.lnz = (int)nb[2];
    // the base layout (slots, leaves, tiles) lives on the device only while the apron blocks
    // are filled from it (avr_vdb.h "Apron layout"): a lookup then reads one slot and one block
    std::vector<int> aslot;
    std::vector<long long> list;
    avr::vdb::build_apron_slots(slot.data(), base.lnx, base.lny, base.lnz, G->tile_value, G->n_tiles, G->background,
                                aslot, list);
    std::vector<float> consts((size_t)G->n_tiles + 1);
    for (int t = 0; t < G->n_tiles; ++t) consts[t] = G->tile_value[t];
    consts[G->n_tiles] = G->background;
    // (declared after the host vectors: it drains the stream before they go, on every return)
    Arena<> tmp(c->stream);
    const size_t nleaf = (size_t)G->n_leaves * 512;
    const auto rSlot = tmp.reserve<int>(slot.size());
    const auto rLeaves = tmp.reserve<float>(nleaf);
    const auto rTiles = tmp.reserve<float>((size_t)G->n_tiles);
    const auto rList = tmp.reserve<long long>(list.size());
    HIP_TRY(tmp.commit());
    HIP_TRY(hipMemcpyAsync(tmp.get(rSlot), slot.data(), slot.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (nleaf)
        HIP_TRY(hipMemcpyAsync(tmp.get(rLeaves), G->leaf_values, nleaf * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (G->n_tiles)
        HIP_TRY(hipMemcpyAsync(tmp.get(rTiles), G->tile_value, G->n_tiles * sizeof(float), hipMemcpyHostToDevice,
                               c->stream));
    base.slot = tmp.get(rSlot);
    base.leaves = tmp.get(rLeaves);
    base.tiles = tmp.get(rTiles);
    HIP_TRY(c->d_vdb_slot[k].alloc(aslot.size()));
    HIP_TRY(hipMemcpyAsync(c->d_vdb_slot[k].get(), aslot.data(), aslot.size() * sizeof(int), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(c->d_vdb_tiles[k].alloc(consts.size()));
    HIP_TRY(hipMemcpyAsync(c->d_vdb_tiles[k].get(), consts.data(), consts.size() * sizeof(float), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(c->d_vdb_leaves[k].alloc(std::max<size_t>(list.size(), 1) * avr::vdb::kApronVals));
    if (!list.empty()) {
        HIP_TRY(hipMemcpyAsync(tmp.get(rList), list.data(), list.size() * sizeof(long long), hipMemcpyHostToDevice,
                               c->stream));
        const long long nl = (long long)list.size();
        const int nblk = (int)std::min<long long>(nl, 1 << 20);
        hipLaunchKernelGGL(avr::k_vdb_apron, dim3(nblk), dim3(256), 0, c->stream, base, tmp.get(rList), nl,
                           c->d_vdb_leaves[k].get());
        HIP_TRY(hipGetLastError());
    }
    // the host vectors and the base layout die here: finish the copies and the fill first
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->vdb_napron[k] = (long long)list.size();
    g.slot = c->d_vdb_slot[k].get();
    g.blocks = c->d_vdb_leaves[k].get();
    g.consts = c->d_vdb_tiles[k].get();
    g.ox = base.ox; g.oy = base.oy; g.oz = base.oz;
    g.lnx = base.lnx; g.lny = base.lny; g.lnz = base.lnz;
    return AVR_OK;
}

// (Re)build the current medium's majorant grid at resolution mres on the device:
// GridMedium MaxValue per cell (media.cpp:229-246), RGBGridMedium's sigma scale x (max
// sigma_a + max sigma_s) (media.cpp:339-378), NanoVDBMedium's slop-widened cell maxima
// (media.cpp:585-613); Homogeneous / Cloud: one segment with majorant 1.
int build_majorant(avr_context *c, const int mres[3]) {
    avr::DevMedium &m = c->med;
    const int type = m.type;
    c->d_majorant.reset();
    const int nm = mres[0] * mres[1] * mres[2];
    c->d_occ.reset();
    m.occ = nullptr;
    // nm cells + one trailing 0: the read target of empty cells under the occupancy level
    HIP_TRY(c->d_majorant.alloc((size_t)nm + 1));
    float *const d_majorant = c->d_majorant.get();
    HIP_TRY(hipMemsetAsync(d_majorant + nm, 0, sizeof(float), c->stream));
    for (int i = 0; i < 3; ++i) {
        m.mres[i] = mres[i];
        m.fres[i] = (float)mres[i];
        m.fresm1[i] = (float)(mres[i] - 1);
    }
    if (type == 0) {
        hipLaunchKernelGGL(avr::k_majorant, dim3(nm), dim3(256), 0, c->stream, m.density, m.nx, m.ny, m.nz, mres[0],
                           mres[1], mres[2], d_majorant);
        HIP_TRY(hipGetLastError());
    } else if (type == 4) {
        hipLaunchKernelGGL(avr::k_majorant_rgb, dim3(nm), dim3(256), 0, c->stream, m.rgb_a, m.rgb_s, m.nx, m.ny, m.nz,
                           mres[0], mres[1], mres[2], m.rgb_sigma_scale, d_majorant);
        HIP_TRY(hipGetLastError());
    } else if (type == 3) {
        const int *b = c->vdb_ibbox;
        hipLaunchKernelGGL(avr::k_majorant_vdb, dim3(nm), dim3(256), 0, c->stream, m.vdb,
                           make_float3(m.bmin[0], m.bmin[1], m.bmin[2]), make_float3(m.bmax[0], m.bmax[1], m.bmax[2]),
                           make_int4(b[0], b[1], b[2], 0), make_int4(b[3], b[4], b[5], 0), mres[0], mres[1], mres[2],
                           d_majorant);
        HIP_TRY(hipGetLastError());
        const int nw = (nm + 63) / 64;
        if (c->majorant_occupancy && nw <= avr::kOccWords) {
            HIP_TRY(c->d_occ.alloc((size_t)nw));
            hipLaunchKernelGGL(avr::k_majorant_occupancy, dim3((nw + 255) / 256), dim3(256), 0, c->stream,
                               d_majorant, nm, c->d_occ.get(), nw);
            HIP_TRY(hipGetLastError());
            m.occ = c->d_occ.get();
        }
    } else {   // single segment, sigma_maj = sigma_t * 1 (density <= 1 for the cloud)
        const float one = 1.f;
        HIP_TRY(hipMemcpyAsync(d_majorant, &one, sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    m.majorant = d_majorant;
    return AVR_OK;
}

int medium_common(avr_context *c, const float *d_density, int nx, int ny, int nz, const float bounds[6],
                  const float rfm[16], const float mfr[16], const float *sigma_a, const float *sigma_s, float g,
                  const float *Le, const float *Lescale, int lnx, int lny, int lnz, const int mres[3],
                  int type = 0, const float cloud[3] = nullptr) {
    if (!affine(rfm) || !affine(mfr)) return fail(AVR_ERR_ARG, "medium transforms must be affine");
    if (!sigma_a || !sigma_s) return fail(AVR_ERR_ARG, "sigma_a/sigma_s tables required");
    if (mres[0] < 1 || mres[1] < 1 || mres[2] < 1) return fail(AVR_ERR_ARG, "bad majorant resolution");
    if (Lescale && (lnx < 1 || lny < 1 || lnz < 1)) return fail(AVR_ERR_ARG, "bad Lescale grid");
    int rc;
    if ((rc = upload_table(c->d_sigma_a, sigma_a, avr::kNTable, c->stream))) return rc;
    if ((rc = upload_table(c->d_sigma_s, sigma_s, avr::kNTable, c->stream))) return rc;
    // Le and LeScale are always resident: a temperature grid attached later makes the medium
    // emissive without an Le spectrum (zeros), and LeScale defaults to pbrt's 1^3 {LeNorm}
    // grid with LeNorm = 1 (media.cpp:288-296)
    static const float zeros[avr::kNTable] = {};
    static const float one = 1.f;
    if ((rc = upload_table(c->d_Le, Le ? Le : zeros, avr::kNTable, c->stream))) return rc;
    if (!Lescale) { Lescale = &one; lnx = lny = lnz = 1; }
    if ((rc = upload_table(c->d_lescale, Lescale, (size_t)lnx * lny * lnz, c->stream))) return rc;
    avr::DevMedium &m = c->med;
    if (type != 3) free_vdb(c);
    if (type != 4) free_rgb(c);
    c->d_temperature.reset();
    m.temperature = nullptr;
    m.temp_scale = 1.f;
    m.temp_offset = 0.f;
    m.type = type;
    m.boundary = 0;   // the bounds box until avr_medium_boundary_sphere
    m.trace = nullptr;
    m.trace_count = nullptr;
    m.trace_cap = 0;
    m.cloud_density = cloud ? cloud[0] : 0.f;
    m.cloud_wispiness = cloud ? cloud[1] : 0.f;
    m.cloud_frequency = cloud ? cloud[2] : 0.f;
    m.density = d_density;
    m.nx = nx; m.ny = ny; m.nz = nz;
    for (int i = 0; i < 3; ++i) { m.bmin[i] = bounds[i]; m.bmax[i] = bounds[3 + i]; m.mres[i] = mres[i]; }
    m.unit_box = (m.bmax[0] - m.bmin[0] == 1.f && m.bmax[1] - m.bmin[1] == 1.f && m.bmax[2] - m.bmin[2] == 1.f) ? 1 : 0;
    copy_xf(m.render_from_medium, rfm);
    copy_xf(m.medium_from_render, mfr);
    m.sigma_a = c->d_sigma_a.get();
    m.sigma_s = c->d_sigma_s.get();
    m.g = g;
    m.hg = avr::hg_consts(g);
    m.fn[0] = (float)nx;
    m.fn[1] = (float)ny;
    m.fn[2] = (float)nz;
    c->gray = true;
    for (int i = 1; i < avr::kNTable; ++i) c->gray &= sigma_a[i] == sigma_a[0] && sigma_s[i] == sigma_s[0];
    c->med.gray_sigma_a = sigma_a[0];
    c->med.gray_sigma_s = sigma_s[0];
    // isEmissive = Le_spec.MaxValue() > 0 (media.cpp:238)
    bool emissive = false;
    if (Le) for (int i = 0; i < avr::kNTable; ++i) emissive |= Le[i] > 0;
    m.emissive = emissive ? 1 : 0;
    m.Le = c->d_Le.get();
    m.lescale = c->d_lescale.get();
    m.lnx = lnx; m.lny = lny; m.lnz = lnz;
    if ((rc = build_majorant(c, mres))) return rc;
    c->d_fat.reset();
    c->d_brick.reset();
    m.fat = nullptr;
    m.brick = nullptr;
    m.nb[0] = m.nb[1] = m.nb[2] = 0;
    if (c->grid_layout == 2 && type == 0) {
        // bricked copy: 8^3 base voxels + apron per brick (k_brickify), 1.42x the grid
        const int nb[3] = {(nx + 8) / 8, (ny + 8) / 8, (nz + 8) / 8};
        const long long nbricks = (long long)nb[0] * nb[1] * nb[2];
        HIP_TRY(c->d_brick.alloc_if_room((size_t)nbricks * avr::kBrickFloats));
        if (c->d_brick) {
            hipLaunchKernelGGL(avr::k_brickify, dim3(blocks_for(nbricks * avr::kBrickFloats, 256, 256 * 64)), dim3(256), 0,
                               c->stream, d_density, nx, ny, nz, nb[0], nb[1], nbricks, c->d_brick.get());
            HIP_TRY(hipGetLastError());
            m.brick = c->d_brick.get();
            for (int a = 0; a < 3; ++a) m.nb[a] = nb[a];
        }
    }
    if (c->grid_layout == 1 && type == 0) {
        const size_t nfat = (size_t)(nx + 1) * (ny + 1) * (nz + 1);
        // 32 B (two float4) per voxel corner, when HBM has them to spare
        HIP_TRY(c->d_fat.alloc_if_room(2 * nfat));
        if (c->d_fat) {
            hipLaunchKernelGGL(avr::k_fatten, dim3(blocks_for((long long)nfat, 256, 256 * 64)), dim3(256), 0,
                               c->stream, d_density, nx, ny, nz, c->d_fat.get());
            HIP_TRY(hipGetLastError());
            m.fat = c->d_fat.get();
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->has_medium = true;
    return AVR_OK;
}

}  // namespace

extern "C" {

const char *avr_last_error(void) { return g_err.c_str(); }


// Setup calls replace or free device buffers that queued work on the context's stream may
// still read, and readbacks through hipMemcpy (the null stream) do not order against a
// non-blocking stream: both first drain the context's stream.
#define AVR_QUIESCE(c)                                                                              \
    do {                                                                                            \
        if (c) ++(c)->cfg_gen;   /* camera records made ahead are not taken across this call */      \
        if ((c) && (c)->stream) {                                                                   \
            hipError_t qe_ = hipStreamSynchronize((c)->stream);                                     \
            if (qe_ == hipSuccess && (c)->tstream) qe_ = hipStreamSynchronize((c)->tstream);        \
            if (qe_ != hipSuccess) return fail(AVR_ERR_HIP, std::string("stream: ") + hipGetErrorString(qe_)); \
        }                                                                                           \
    } while (0)

int avr_context_create(int device, long long max_paths, avr_context **out) {
    if (!out) return fail(AVR_ERR_ARG, "null out");
    // path ids (s * pixels + pixel) are 32-bit in the kernels: passes hold < 2^31 paths
    if (max_paths > INT_MAX) return fail(AVR_ERR_ARG, "max_paths above 2^31 - 1 (32-bit path ids)");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(AVR_ERR_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    auto *c = new avr_context();
    c->device = device;
    if (max_paths > 0) c->max_paths = max_paths, c->max_paths_set = true;
    // the path stream at the greatest priority, the side stream (ptab_spec's tables built
    // ahead) at the least, so the dispatcher serves the side stream's blocks only from CUs the
    // path kernels leave free
    int prLeast = 0, prGreatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&prLeast, &prGreatest);
    // (a chain, not HIP_TRY: the context made so far is destroyed on a failure)
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->own_stream.h, hipStreamNonBlocking, prGreatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->tstream.h, hipStreamNonBlocking, prLeast);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_cam.h, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_tab.h, hipEventDisableTiming);
    if (e != hipSuccess) { (void)avr_context_destroy(c); return fail(AVR_ERR_HIP, hipGetErrorString(e)); }
    c->stream = c->own_stream;
    if (c->d_counts.alloc(4) != hipSuccess || c->d_stats.alloc(avr::kNumStats + 8) != hipSuccess ||
        hipHostMalloc((void **)&c->h_count.h, sizeof(int) * 4) != hipSuccess) {
        (void)avr_context_destroy(c);
        return fail(AVR_ERR_HIP, "context allocation failed");
    }
    if (c->set.alloc_heads() != hipSuccess ||
        hipMemset(c->d_stats.get(), 0, sizeof(unsigned long long) * (avr::kNumStats + 8)) != hipSuccess) {
        (void)avr_context_destroy(c);
        return fail(AVR_ERR_HIP, "context allocation failed");
    }
    {
        // persistent grid per k_paths variant: every admitted block resident. No block ever
        // waits on another (work is pulled from counters), so the API's answer is safe as is.
        // The variants differ in VGPRs (gray: 3 waves/SIMD, 4-wavelength: 2), so each gets
        // its own grid.
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
            (void)avr_context_destroy(c);
            return fail(AVR_ERR_HIP, "device query failed");
        }
        c->num_cus = prop.multiProcessorCount;
#define AVR_KP_ENTRY(em, gr, zs, med, im, fa)                                                    \
    c->kpaths[avr::kp::slot_of(em, gr, zs, med, im, fa)] = avr::k_paths<em, gr, zs, med, im, fa>; \
    c->kpaths_name[avr::kp::slot_of(em, gr, zs, med, im, fa)] = AVR_KP_NAME(em, gr, zs, med, im, fa);
        AVR_KP_ALL(AVR_KP_ENTRY)
#undef AVR_KP_ENTRY
        avr::kp::alias_rgb_gray(c->kpaths);
        avr::kp::alias_rgb_gray(c->kpaths_name);
        for (int k = 0; k < avr_context::kNumPaths; ++k) {
            int blocksPerCU = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocksPerCU, c->kpaths[k], 256, 0) != hipSuccess) {
                (void)avr_context_destroy(c);
                return fail(AVR_ERR_HIP, "occupancy query failed");
            }
            c->paths_grid[k] = prop.multiProcessorCount * std::max(1, blocksPerCU);
        }
    }
    *out = c;
    return AVR_OK;
}

int avr_set_grid_layout(avr_context *c, int layout) {
    AVR_QUIESCE(c);
    if (!c || layout < 0 || layout > 2) return fail(AVR_ERR_ARG, "grid layout must be 0 (linear), 1 (fat) or 2 (bricked)");
    c->grid_layout = layout;
    return AVR_OK;
}

int avr_grid_layout_active(avr_context *c) { return !c ? 0 : (c->d_fat ? 1 : (c->med.brick ? 2 : 0)); }

int avr_set_dda_budget(avr_context *c, int cells) {
    if (!c || cells < 0) return fail(AVR_ERR_ARG, "DDA budget must be >= 1 cell (0: default)");
    c->dda_budget = cells;
    return AVR_OK;
}

int avr_set_refill_min(avr_context *c, int lanes) {
    if (!c || lanes < 0 || lanes > 64) return fail(AVR_ERR_ARG, "refill threshold must be 0..64 lanes (0 = default)");
    c->refill_min = lanes;
    return AVR_OK;
}

int avr_set_refill_batch(avr_context *c, int lanes) {
    if (!c || lanes < 0 || lanes > 64) return fail(AVR_ERR_ARG, "refill batch must be 0..64 lanes (0 = default)");
    c->refill_batch = lanes;
    return AVR_OK;
}

int avr_set_render_mode(avr_context *c, int mode) {
    AVR_QUIESCE(c);
    if (!c || (mode != 0 && mode != 1)) return fail(AVR_ERR_ARG, "render mode must be 0 (replay) or 1 (fast)");
    c->render_mode = mode;
    return AVR_OK;
}

int avr_set_ray_binning(avr_context *c, int on) {
    AVR_QUIESCE(c);
    if (!c || (on != 0 && on != 1)) return fail(AVR_ERR_ARG, "ray binning must be 0 or 1");
    c->ray_binning = on;
    return AVR_OK;
}

int avr_set_pass_table_ahead(avr_context *c, int on) {
    AVR_QUIESCE(c);
    if (!c || (on != 0 && on != 1)) return fail(AVR_ERR_ARG, "pass table ahead must be 0 or 1");
    c->ptab_spec = on;
    c->look.invalidate();   // (the side stream is idle after the quiesce)
    return AVR_OK;
}

int avr_set_pass_overlap(avr_context *c, int on) {
    AVR_QUIESCE(c);
    if (!c || (on != 0 && on != 1)) return fail(AVR_ERR_ARG, "pass overlap must be 0 or 1");
    c->pass_overlap = on;
    c->look.invalidate();
    return AVR_OK;
}

int avr_pass_overlap_active(avr_context *c) { return c && c->last.overlap ? 1 : 0; }

int avr_set_majorant_occupancy(avr_context *c, int on) {
    AVR_QUIESCE(c);
    if (!c || (on != 0 && on != 1)) return fail(AVR_ERR_ARG, "majorant occupancy must be 0 or 1");
    HIP_TRY(hipSetDevice(c->device));
    c->majorant_occupancy = on;
    if (c->has_medium) {   // rebuild the current majorant (same values) with / without the level
        const int r[3] = {c->med.mres[0], c->med.mres[1], c->med.mres[2]};
        return build_majorant(c, r);
    }
    return AVR_OK;
}

int avr_set_kernel_mode(avr_context *c, int mode) {
    if (!c || (mode != 0 && mode != 1)) return fail(AVR_ERR_ARG, "kernel mode must be 0 (persistent) or 1 (wavefront)");
    c->kernel_mode = mode;
    return AVR_OK;
}

int avr_context_destroy(avr_context *c) {
    if (!c) return AVR_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->tstream) (void)hipStreamSynchronize(c->tstream);
    release_comms(c);
    delete c;   // the device buffers, then the events and streams (avr_context's member order)
    return AVR_OK;
}

int avr_set_stream(avr_context *c, void *s) {
    // work built ahead on the side stream is ordered against the stream it was enqueued beside
    AVR_QUIESCE(c);
    if (!c) return fail(AVR_ERR_ARG, "null context");
    c->look.invalidate();
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return AVR_OK;
}

int avr_medium_grid(avr_context *c, const float *density, int nx, int ny, int nz, const float bounds[6],
                    const float rfm[16], const float mfr[16], const float *sigma_a, const float *sigma_s, float g,
                    const float *Le, const float *Lescale, int lnx, int lny, int lnz, const int mres[3]) {
    AVR_QUIESCE(c);
    if (!c || !density || nx < 1 || ny < 1 || nz < 1) return fail(AVR_ERR_ARG, "bad grid");
    HIP_TRY(hipSetDevice(c->device));
    c->d_density_owned.reset();
    const size_t n = (size_t)nx * ny * nz;
    if (n > (size_t)INT32_MAX) return fail(AVR_ERR_ARG, "grid too large for int32 indexing (containers.h:834)");
    HIP_TRY(c->d_density_owned.alloc(n));
    HIP_TRY(hipMemcpyAsync(c->d_density_owned.get(), density, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return medium_common(c, c->d_density_owned.get(), nx, ny, nz, bounds, rfm, mfr, sigma_a, sigma_s, g, Le, Lescale, lnx,
                         lny, lnz, mres);
}

int avr_medium_grid_device(avr_context *c, const float *d_density, int nx, int ny, int nz, const float bounds[6],
                           const float rfm[16], const float mfr[16], const float *sigma_a, const float *sigma_s,
                           float g, const float *Le, const float *Lescale, int lnx, int lny, int lnz,
                           const int mres[3]) {
    AVR_QUIESCE(c);
    if (!c || !d_density || nx < 1 || ny < 1 || nz < 1) return fail(AVR_ERR_ARG, "bad grid");
    if ((size_t)nx * ny * nz > (size_t)INT32_MAX) return fail(AVR_ERR_ARG, "grid too large for int32 indexing");
    HIP_TRY(hipSetDevice(c->device));
    c->d_density_owned.reset();
    return medium_common(c, d_density, nx, ny, nz, bounds, rfm, mfr, sigma_a, sigma_s, g, Le, Lescale, lnx, lny, lnz,
                         mres);
}

int avr_medium_temperature(avr_context *c, const float *temperature, float temperature_scale,
                           float temperature_offset) {
    AVR_QUIESCE(c);
    if (!c || !temperature) return fail(AVR_ERR_ARG, "null temperature grid");
    if (!c->has_medium || c->med.type != 0) return fail(AVR_ERR_STATE, "temperature needs a grid medium first");
    if (!c->med.Le || !c->med.lescale) return fail(AVR_ERR_STATE, "medium emission tables missing");
    if (c->med.Le && c->med.emissive && !c->med.temperature)
        return fail(AVR_ERR_ARG, "both \"Le\" and \"temperature\" given (media.cpp:283-284)");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)c->med.nx * c->med.ny * c->med.nz;
    HIP_TRY(c->d_temperature.alloc(n));
    HIP_TRY(hipMemcpy(c->d_temperature.get(), temperature, n * sizeof(float), hipMemcpyHostToDevice));
    c->med.temperature = c->d_temperature.get();
    c->med.temp_scale = temperature_scale;
    c->med.temp_offset = temperature_offset;
    c->med.emissive = 1;   // isEmissive = temperatureGrid ? true : ... (media.cpp:238)
    return AVR_OK;
}

int avr_medium_homogeneous(avr_context *c, const float bounds[6], const float rfm[16], const float mfr[16],
                           const float *sigma_a, const float *sigma_s, float g, const float *Le) {
    AVR_QUIESCE(c);
    if (!c || !bounds || !rfm || !mfr) return fail(AVR_ERR_ARG, "null medium argument");
    HIP_TRY(hipSetDevice(c->device));
    static const float one = 1.f;
    const int mres[3] = {1, 1, 1};
    return medium_common(c, nullptr, 1, 1, 1, bounds, rfm, mfr, sigma_a, sigma_s, g, Le, Le ? &one : nullptr, 1, 1, 1,
                         mres, 1, nullptr);
}

int avr_medium_cloud(avr_context *c, const float bounds[6], const float rfm[16], const float mfr[16],
                     const float *sigma_a, const float *sigma_s, float g, float density, float wispiness,
                     float frequency) {
    AVR_QUIESCE(c);
    if (!c || !bounds || !rfm || !mfr) return fail(AVR_ERR_ARG, "null medium argument");
    HIP_TRY(hipSetDevice(c->device));
    const int mres[3] = {1, 1, 1};
    const float cloud[3] = {density, wispiness, frequency};
    return medium_common(c, nullptr, 1, 1, 1, bounds, rfm, mfr, sigma_a, sigma_s, g, nullptr, nullptr, 1, 1, 1, mres,
                         2, cloud);
}

int avr_medium_nanovdb(avr_context *c, const avr_vdb_grid *density, const avr_vdb_grid *temperature, const float rfm[16],
                       const float mfr[16], const float *sigma_a, const float *sigma_s, float g, float Lescale,
                       float temperature_offset, float temperature_scale) {
    AVR_QUIESCE(c);
    if (!c || !density || !rfm || !mfr) return fail(AVR_ERR_ARG, "null medium argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_vdb(c);
    int rc;
    avr::vdb::Apron gd{}, gt{};
    if ((rc = upload_vdb(c, density, 0, gd))) return rc;
    if (temperature && (rc = upload_vdb(c, temperature, 1, gt))) return rc;
    // bounds: density world bbox, union the temperature grid's (media.cpp:531-549)
    double lo[3], hi[3];
    vdb_world_bbox(density, lo, hi);
    float bounds[6];
    for (int a = 0; a < 3; ++a) { bounds[a] = (float)lo[a]; bounds[3 + a] = (float)hi[a]; }
    if (temperature) {
        vdb_world_bbox(temperature, lo, hi);
        for (int a = 0; a < 3; ++a) {
            bounds[a] = std::min(bounds[a], (float)lo[a]);
            bounds[3 + a] = std::max(bounds[3 + a], (float)hi[a]);
        }
    }
    for (int a = 0; a < 6; ++a) c->vdb_ibbox[a] = density->index_bbox[a];
    c->med.vdb = gd;
    c->med.vdb_temp = gt;
    const int mres[3] = {64, 64, 64};   // majorantGrid(Bounds3f(), {64, 64, 64}) (media.cpp:520)
    if ((rc = medium_common(c, nullptr, 1, 1, 1, bounds, rfm, mfr, sigma_a, sigma_s, g, nullptr, nullptr, 1, 1, 1, mres,
                            3, nullptr)))
        return rc;
    // the density grid's fat copy (avr_set_grid_layout 1, as for GridMedium): 32 B per base voxel
    // of every apron block, when it fits in free HBM with 8 GiB to spare
    if (c->grid_layout == 1 && c->vdb_napron[0] > 0) {
        const size_t nfat = (size_t)c->vdb_napron[0] * 512;
        HIP_TRY(c->d_fat.alloc_if_room(2 * nfat));
        if (c->d_fat) {
            hipLaunchKernelGGL(avr::k_vdb_fat, dim3(blocks_for((long long)nfat, 256, 256 * 64)), dim3(256), 0, c->stream,
                               c->med.vdb.blocks, c->vdb_napron[0], c->d_fat.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->med.vdb.fat = reinterpret_cast<const float *>(c->d_fat.get());
        }
    }
    c->med.vdb_lescale = Lescale;
    c->med.temp_offset = temperature_offset;
    c->med.temp_scale = temperature_scale;
    c->med.emissive = temperature ? 1 : 0;
    return AVR_OK;
}

static int medium_rgbgrid(avr_context *c, int nx, int ny, int nz, const float bounds[6], const float rfm[16],
                          const float mfr[16], const float *sigma_a, const float *sigma_s, float sigma_scale, float g,
                          const float *Le, const float *illuminant, float Le_scale, bool on_device) {
    AVR_QUIESCE(c);
    if (!c || !bounds || !rfm || !mfr) return fail(AVR_ERR_ARG, "null medium argument");
    if (nx < 1 || ny < 1 || nz < 1) return fail(AVR_ERR_ARG, "bad grid");
    if (!sigma_a && !sigma_s)
        return fail(AVR_ERR_ARG, "RGB grid requires \"sigma_a\" and/or \"sigma_s\" (media.cpp:404-406)");
    if (Le && !sigma_a) return fail(AVR_ERR_ARG, "RGB grid requires \"sigma_a\" if \"Le\" given (media.cpp:418-419)");
    if (Le && !illuminant) return fail(AVR_ERR_ARG, "Le needs the colour space's illuminant table");
    const size_t n = (size_t)nx * ny * nz;
    if (n > (size_t)INT32_MAX) return fail(AVR_ERR_ARG, "grid too large for int32 indexing");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_rgb(c);
    const float *src[3] = {sigma_a, sigma_s, Le};
    const float4 *grid[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; ++k) {
        if (!src[k]) continue;
        if (on_device) {   // the caller's device arrays, adopted (not copied)
            grid[k] = reinterpret_cast<const float4 *>(src[k]);
            continue;
        }
        HIP_TRY(c->d_rgb[k].alloc(n));
        HIP_TRY(hipMemcpyAsync(c->d_rgb[k].get(), src[k], n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        grid[k] = c->d_rgb[k].get();
    }
    int rc;
    if (Le && (rc = upload_table(c->d_illum, illuminant, avr::kNTable, c->stream))) return rc;
    c->med.rgb_a = grid[0];
    c->med.rgb_s = grid[1];
    c->med.rgb_le = grid[2];
    c->med.illuminant = c->d_illum.get();
    c->med.rgb_sigma_scale = sigma_scale;
    c->med.rgb_le_scale = Le_scale;
    // SampleRay's sigma_t = 1 (media.h:417): tables {1} + {0} make the segments' sigma_maj the
    // majorant value itself; SamplePoint reads the RGB grids instead of the tables
    static float ones[avr::kNTable], zeros[avr::kNTable];
    for (int i = 0; i < avr::kNTable; ++i) ones[i] = 1.f;
    const int mres[3] = {16, 16, 16};   // majorantGrid(bounds, {16, 16, 16}) (media.cpp:352)
    if ((rc = medium_common(c, nullptr, nx, ny, nz, bounds, rfm, mfr, ones, zeros, g, nullptr, nullptr, 1, 1, 1, mres,
                            4, nullptr)))
        return rc;
    c->med.emissive = (Le && Le_scale > 0) ? 1 : 0;   // IsEmissive (media.h:374)
    return AVR_OK;
}

int avr_medium_rgbgrid(avr_context *c, int nx, int ny, int nz, const float bounds[6], const float rfm[16],
                       const float mfr[16], const float *sigma_a, const float *sigma_s, float sigma_scale, float g,
                       const float *Le, const float *illuminant, float Le_scale) {
    return medium_rgbgrid(c, nx, ny, nz, bounds, rfm, mfr, sigma_a, sigma_s, sigma_scale, g, Le, illuminant, Le_scale,
                          false);
}

int avr_medium_rgbgrid_device(avr_context *c, int nx, int ny, int nz, const float bounds[6], const float rfm[16],
                              const float mfr[16], const float *d_sigma_a, const float *d_sigma_s, float sigma_scale,
                              float g, const float *d_Le, const float *illuminant, float Le_scale) {
    return medium_rgbgrid(c, nx, ny, nz, bounds, rfm, mfr, d_sigma_a, d_sigma_s, sigma_scale, g, d_Le, illuminant,
                          Le_scale, true);
}

int avr_generate_rgb_explosion(avr_context *c, float *d_sigma_a, float *d_sigma_s, float *d_Le, int n, long long first,
                               long long count) {
    if (!c || !d_sigma_a || !d_sigma_s || !d_Le || n < 1 || count < 0 || first < 0 ||
        first + count > (long long)n * n * n)
        return fail(AVR_ERR_ARG, "bad rgb explosion args");
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(avr::k_rgb_explosion, dim3(blocks_for(count, 256, 256 * 32)), dim3(256), 0, c->stream,
                       reinterpret_cast<float4 *>(d_sigma_a), reinterpret_cast<float4 *>(d_sigma_s),
                       reinterpret_cast<float4 *>(d_Le), n, first, count);
    HIP_TRY(hipGetLastError());
    return AVR_OK;
}

int avr_medium_bounds(avr_context *c, float bounds[6]) {
    AVR_QUIESCE(c);
    if (!c || !c->has_medium || !bounds) return fail(AVR_ERR_STATE, "no medium");
    for (int a = 0; a < 3; ++a) { bounds[a] = c->med.bmin[a]; bounds[3 + a] = c->med.bmax[a]; }
    return AVR_OK;
}

int avr_generate_cloud(avr_context *c, float *d_out, int n, long long first, long long count, float density,
                       float wispiness, float frequency) {
    if (!c || !d_out || n < 1 || count < 0) return fail(AVR_ERR_ARG, "bad cloud args");
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(avr::k_cloud, dim3(blocks_for(count, 256, 256 * 32)), dim3(256), 0, c->stream, d_out, n, first,
                       count, density, wispiness, frequency);
    HIP_TRY(hipGetLastError());
    return AVR_OK;
}

int avr_read_majorant(avr_context *c, float *out) {
    AVR_QUIESCE(c);
    if (!c || !c->has_medium || !out) return fail(AVR_ERR_STATE, "no medium");
    const int nm = c->med.mres[0] * c->med.mres[1] * c->med.mres[2];
    HIP_TRY(hipMemcpyAsync(out, c->d_majorant.get(), nm * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_medium_boundary_sphere(avr_context *c, const float center[3], float radius) {
    AVR_QUIESCE(c);
    if (!c || !c->has_medium) return fail(AVR_ERR_STATE, "no medium");
    if (radius > 0 && !center) return fail(AVR_ERR_ARG, "null sphere centre");
    if (!(radius <= 0 || std::isfinite(radius))) return fail(AVR_ERR_ARG, "sphere radius must be finite");
    c->med.boundary = radius > 0 ? 1 : 0;
    for (int i = 0; i < 3; ++i) c->med.sph[i] = radius > 0 ? center[i] : 0.f;
    c->med.sph[3] = radius > 0 ? radius : 0.f;
    return AVR_OK;
}

int avr_medium_boundary_convex(avr_context *c, const float *planes, int n_planes) {
    AVR_QUIESCE(c);
    if (!c || !c->has_medium) return fail(AVR_ERR_STATE, "no medium");
    if (n_planes < 0 || n_planes > 256 || (n_planes > 0 && !planes))
        return fail(AVR_ERR_ARG, "convex interface: 0..256 planes {nx, ny, nz, h}");
    for (int i = 0; i < 4 * n_planes; ++i)
        if (!std::isfinite(planes[i])) return fail(AVR_ERR_ARG, "convex interface planes must be finite");
    HIP_TRY(hipSetDevice(c->device));
    c->d_planes.reset();
    c->med.planes = nullptr;
    c->med.n_planes = 0;
    if (n_planes == 0) {
        if (c->med.boundary == 2) c->med.boundary = 0;
        return AVR_OK;
    }
    HIP_TRY(c->d_planes.alloc((size_t)n_planes));
    HIP_TRY(hipMemcpyAsync(c->d_planes.get(), planes, 4 * sizeof(float) * n_planes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->med.planes = c->d_planes.get();
    c->med.n_planes = n_planes;
    c->med.boundary = 2;
    return AVR_OK;
}

int avr_record_lookups(avr_context *c, void *d_points, long long cap, void *d_count) {
    AVR_QUIESCE(c);
    if (!c || !c->has_medium) return fail(AVR_ERR_STATE, "no medium");
    if (d_points && (cap < 0 || !d_count)) return fail(AVR_ERR_ARG, "lookup trace needs a capacity and a counter");
    c->med.trace = (float4 *)d_points;
    c->med.trace_count = d_points ? (unsigned long long *)d_count : nullptr;
    c->med.trace_cap = d_points ? cap : 0;
    return AVR_OK;
}

int avr_density_fetch(avr_context *c, const void *d_points, long long n, float *d_out, float *ms) {
    AVR_QUIESCE(c);
    if (!c || !c->has_medium || c->med.type != 0) return fail(AVR_ERR_STATE, "density fetch needs a GridMedium");
    if (n < 0 || (n > 0 && (!d_points || !d_out))) return fail(AVR_ERR_ARG, "bad density fetch batch");
    HIP_TRY(hipSetDevice(c->device));
    avr::devmem::Event e0, e1;
    HIP_TRY(hipEventCreate(&e0.h));
    HIP_TRY(hipEventCreate(&e1.h));
    const int blocks = (int)std::min<long long>((n + 255) / 256, 256LL * 64);
    HIP_TRY(hipEventRecord(e0, c->stream));
    if (n > 0)
        hipLaunchKernelGGL(avr::k_density_fetch, dim3(blocks), dim3(256), 0, c->stream, c->med,
                           (const float4 *)d_points, n, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e1, c->stream));
    HIP_TRY(hipEventSynchronize(e1));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t;
    return AVR_OK;
}

int avr_vdb_fetch(avr_context *c, int grid, const void *d_points, long long n, float *d_out, float *ms) {
    AVR_QUIESCE(c);
    if (!c || !c->has_medium || c->med.type != 3) return fail(AVR_ERR_STATE, "vdb fetch needs a NanoVDBMedium");
    if (grid != 0 && grid != 1) return fail(AVR_ERR_ARG, "vdb fetch: grid must be 0 (density) or 1 (temperature)");
    if (grid == 1 && !c->d_vdb_slot[1]) return fail(AVR_ERR_STATE, "vdb fetch: the medium has no temperature grid");
    if (n < 0 || (n > 0 && (!d_points || !d_out))) return fail(AVR_ERR_ARG, "bad vdb fetch batch");
    HIP_TRY(hipSetDevice(c->device));
    avr::devmem::Event e0, e1;
    HIP_TRY(hipEventCreate(&e0.h));
    HIP_TRY(hipEventCreate(&e1.h));
    const int blocks = (int)std::min<long long>((n + 255) / 256, 256LL * 64);
    HIP_TRY(hipEventRecord(e0, c->stream));
    if (n > 0)
        hipLaunchKernelGGL(avr::k_vdb_fetch, dim3(blocks), dim3(256), 0, c->stream, grid ? c->med.vdb_temp : c->med.vdb,
                           (const float4 *)d_points, n, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e1, c->stream));
    HIP_TRY(hipEventSynchronize(e1));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, e0, e1));
    if (ms) *ms = t;
    return AVR_OK;
}

int avr_rgbgrid_probe(avr_context *c, long long n, const float *points, const float *lambda, float *sigma_a4,
                      float *sigma_s4, float *Le4) {
    AVR_QUIESCE(c);
    if (!c || !c->has_medium || c->med.type != 4) return fail(AVR_ERR_STATE, "rgbgrid probe needs an RGBGridMedium");
    if (n < 0 || (n > 0 && (!points || !lambda))) return fail(AVR_ERR_ARG, "bad rgbgrid probe batch");
    if (n == 0) return AVR_OK;
    HIP_TRY(hipSetDevice(c->device));
    Arena<> scratch(c->stream);
    const auto rp = scratch.reserve<float>(3 * (size_t)n), rl = scratch.reserve<float>(4 * (size_t)n);
    const auto ro = scratch.reserve<float>(12 * (size_t)n);
    HIP_TRY(scratch.commit());
    float *dp = scratch.get(rp), *dl = scratch.get(rl), *dout = scratch.get(ro);
    float *host[3] = {sigma_a4, sigma_s4, Le4}, *dev[3];
    for (int k = 0; k < 3; ++k) dev[k] = host[k] ? dout + 4 * (size_t)n * k : nullptr;
    HIP_TRY(hipMemcpyAsync(dp, points, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dl, lambda, 4 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const int blocks = (int)std::min<long long>((n + 255) / 256, 256LL * 64);
    hipLaunchKernelGGL(avr::k_rgb_probe, dim3(blocks), dim3(256), 0, c->stream, c->med, dp, dl, n, dev[0], dev[1], dev[2]);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < 3; ++k)
        if (host[k]) HIP_TRY(hipMemcpyAsync(host[k], dev[k], 4 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_set_majorant_res(avr_context *c, const int res[3]) {
    AVR_QUIESCE(c);
    if (!c || !c->has_medium || !res) return fail(AVR_ERR_STATE, "no medium");
    if (c->med.type == 1 || c->med.type == 2)
        return fail(AVR_ERR_ARG, "homogeneous / cloud media have a single majorant segment");
    if (res[0] < 1 || res[1] < 1 || res[2] < 1 || res[0] > 255 || res[1] > 255 || res[2] > 255)
        return fail(AVR_ERR_ARG, "majorant resolution must be 1..255 per axis");
    HIP_TRY(hipSetDevice(c->device));
    int rc = build_majorant(c, res);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

// The probe loop of the device-side tuners (avr_tune_majorant, avr_tune_walk): render
// [spp_begin, spp_end) after setup(k) for each k < n, twice (k ascending, then descending) —
// plus one untimed render after setup(0) first (the first render after a scene change builds
// one-off tables) — timed with HIP events on the context stream; each candidate's time is the
// faster of its two probes; *bestk = the fastest, ms[k] the times when non-null. The
// film sums are saved before and restored after (also when a probe fails; the first error is
// kept); restore() then re-applies the chosen (or, after a failure, the original) setting.
// prefer >= 0: that candidate (the default schedule) is kept unless the fastest probe beats it
// by more than kProbeNoise — the probes' run-to-run spread — so the choice is reproducible. Its
// time is the fastest probe of every candidate marked in `same` (those that run the very same
// schedule, e.g. refill 0 and refill 32 when 32 is the default), not one noisy probe.
constexpr float kProbeNoise = 0.02f;
extern "C++" {
// avr_film_export_device's inverse: the film's sums from `src`
static int film_import_device(avr_context *c, const double *src) {
    const size_t np = (size_t)c->film.bw * c->film.bh;
    HIP_TRY(hipMemcpyAsync(c->film.rgb_sum, src, 3 * np * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->film.w_sum, src + 3 * np, np * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (c->film.nbuckets > 0)
        HIP_TRY(hipMemcpyAsync(c->film.bucket_sum, src + 4 * np, 2 * np * c->film.nbuckets * sizeof(double),
                               hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}
template <typename Setup, typename Restore>
static int probe_loop(avr_context *c, int n, Setup setup, Restore restore, int spp_begin, int spp_end, int seed,
                      int max_depth, int *bestk, float *ms, int prefer = -1, const std::vector<char> *same = nullptr) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t np = (size_t)c->film.bw * c->film.bh;
    const size_t nd = (4 + 2 * (size_t)std::max(0, c->film.nbuckets)) * np;
    Buffer<double> saved;
    HIP_TRY(saved.alloc(nd));
    int rc = avr_film_export_device(c, saved.get());
    const bool haveSaved = rc == AVR_OK;
    avr::devmem::Event e0, e1;
    if (!rc && (hipEventCreate(&e0.h) != hipSuccess || hipEventCreate(&e1.h) != hipSuccess)) rc = fail(AVR_ERR_HIP, "event");
    float best = -1.f, tPrefer = -1.f;
    *bestk = 0;
    // the probes render one range over and over: no pass table built ahead on the side stream
    // (a probe would wait for the previous one's), restored afterwards
    const int spec0 = c->ptab_spec;
    c->ptab_spec = 0;
    c->look.invalidate();
    // two rounds over the candidates, the second in reverse order, each candidate's time the
    // faster of its two probes (one probe each left 1^3 and 2^3 of fast mode to noise)
    std::vector<float> tmin(n, -1.f);
    for (int it = -1; it < 2 * n && !rc; ++it) {
        const int k = it < 0 ? -1 : (it < n ? it : 2 * n - 1 - it);
        if ((rc = setup(k < 0 ? 0 : k))) break;
        if (hipEventRecord(e0, c->stream) != hipSuccess) { rc = fail(AVR_ERR_HIP, "event record"); break; }
        if ((rc = avr_render(c, spp_begin, spp_end, seed, max_depth))) break;
        if (hipEventRecord(e1, c->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) {
            rc = fail(AVR_ERR_HIP, "event sync");
            break;
        }
        float t = 0.f;
        (void)hipEventElapsedTime(&t, e0, e1);
        if (k >= 0 && (tmin[k] < 0 || t < tmin[k])) tmin[k] = t;
    }
    c->ptab_spec = spec0;
    for (int k = 0; k < n && !rc; ++k) {
        const float t = tmin[k];
        if (ms) ms[k] = t;
        if ((k == prefer || (same && (*same)[k])) && (tPrefer < 0 || t < tPrefer)) tPrefer = t;
        if (best < 0 || t < best) { best = t; *bestk = k; }
    }
    if (!rc && prefer >= 0 && tPrefer >= 0 && tPrefer <= best * (1 + kProbeNoise)) *bestk = prefer;
    const std::string err = g_err;
    const int rcProbe = rc;
    int rcRestore = restore(rc != 0, *bestk);
    if (haveSaved) {   // (restore()'s error comes before the film's)
        const std::string errRestore = g_err;
        const int rcFilm = film_import_device(c, saved.get());
        if (rcRestore) g_err = errRestore;
        else rcRestore = rcFilm;
    }
    if (rcProbe) {
        rc = rcProbe;
        g_err = err;
    } else {
        rc = rcRestore;
    }
    if (!rc) rc = avr_reset_stats(c);
    return rc;
}
}  // extern "C++"

int avr_tune_majorant(avr_context *c, const int *candidates, int n, int spp_begin, int spp_end, int seed,
                      int max_depth, int chosen[3], float *ms) {
    AVR_QUIESCE(c);
    if (!c || !candidates || n < 1 || !chosen) return fail(AVR_ERR_ARG, "null argument");
    if (!c->has_medium || !c->has_film || !c->has_camera) return fail(AVR_ERR_STATE, "scene incomplete");
    if (c->med.type == 1 || c->med.type == 2)
        return fail(AVR_ERR_ARG, "homogeneous / cloud media have a single majorant segment");
    if (spp_end <= spp_begin) return fail(AVR_ERR_ARG, "empty probe sample range");
    for (int k = 0; k < 3 * n; ++k)
        if (candidates[k] < 1 || candidates[k] > 255) return fail(AVR_ERR_ARG, "majorant resolution must be 1..255");
    const int mres0[3] = {c->med.mres[0], c->med.mres[1], c->med.mres[2]};
    int bestk = 0;
    const int rc = probe_loop(
        c, n, [&](int k) { return build_majorant(c, candidates + 3 * k); },
        [&](bool failed, int b) { return build_majorant(c, failed ? mres0 : candidates + 3 * b); }, spp_begin, spp_end,
        seed, max_depth, &bestk, ms);
    if (!rc)
        for (int i = 0; i < 3; ++i) chosen[i] = candidates[3 * bestk + i];
    return rc;
}

// k_paths' effective walk schedule for requested (refill lanes, DDA cells), 0 = the defaults —
// measured optima: refill at 32 idle lanes and 10 DDA cells per iteration for 16^3
// majorants, 32 cells for finer ones; a non-emissive NanoVDB medium (pbrt's 64^3 majorant: ~4x the
// DDA steps of the grid) refills at 20 lanes with 28 cells (S-cloud-1024: 1239 -> 1352
// Msamples/s at 12 / 28 in round 3, 1435 -> 1464 at 16 / 28 in round 5, 1619 -> 1638 at 20 / 28
// in round 6, profiles/r06_walk_sweep.json); an RGBGridMedium (8 sigmoid taps x 4 wavelengths per
// lookup, 2 waves / SIMD) at 16 lanes with 32 cells (C5's RGB explosion: 1770 -> 2094 Msamples/s)
// The third value is the refill batch the kernel takes (Params::refill_batch): the requested one
// (avr_set_refill_batch), else the kind's default. `refill` is the service threshold.
static void walk_schedule(const avr_context *c, int refill, int dda, int *r_eff, int *d_eff, int *b_eff = nullptr) {
    const int mres = std::max(c->med.mres[0], std::max(c->med.mres[1], c->med.mres[2]));
    const bool vdbWalk = c->med.type == 3 && !c->med.emissive && mres > 16;
    const bool rgbWalk = c->med.type == 4;
    // a GridMedium majorant of at most 2 cells per axis (fast mode's tuned 1^3): walks of one
    // or two cells, so the event handlers dominate and larger batches win
    const bool coarse = c->med.type == 0 && mres <= 2;
    // measured optima (profiles/r06_walk_sweep.json for the round-6 kernels: NanoVDB 20 / 28,
    // coarse 48)
    *r_eff = refill > 0 ? refill : (vdbWalk ? 20 : (rgbWalk ? 16 : (coarse ? 48 : 32)));
    *d_eff = dda > 0 ? dda : (vdbWalk ? 28 : (rgbWalk || mres > 16 ? 32 : 10));
    // The refill batch: a gray, non-emissive GridMedium (the headline's 16^3 majorant and the coarse
    // one alike: the parked k_paths<false, true, ...> family)
    // refills whatever waits at every service round (batch 1; plain bench lines against the
    // parent's tuned coupled schedule: S-cloud-1024 3083-3086 -> 3188-3192 Msamples/s, fast mode's
    // 1^3 majorant 4063-4066 -> 4695-4698, profiles/refill_batch_ab.json; batches of 8, 16 or the
    // threshold fall between). The other kinds keep the coupled schedule, a refill at the service
    // threshold with every waiting lane counted towards it (a negative Params value): the NanoVDB
    // walk gains at its default threshold (k_paths 32.14 -> 30.61 ms in one sweep process) but not
    // against the coupled schedule at 12 lanes that the bench's tuner finds (1775-1781 -> 1761-1767),
    // and the rest (emissive or chromatic grids, RGB grids, homogeneous media) are not measured.
    // (the API's values 1..64 cannot name the coupled schedule: a library built with
    // -DAVR_COUPLED_DEFAULT keeps it for every kind, for A/B runs and the probe counters)
#ifdef AVR_COUPLED_DEFAULT
    const bool eager = false;
#else
    const bool eager = c->med.type == 0 && c->gray && !c->med.emissive;
#endif
    if (b_eff) *b_eff = c->refill_batch > 0 ? c->refill_batch : (eager ? 1 : -*r_eff);
}

int avr_tune_walk(avr_context *c, const int *refill, int nr, const int *dda, int nd, int spp_begin, int spp_end,
                  int seed, int max_depth, int chosen[2], float *ms) {
    AVR_QUIESCE(c);
    if (!c || !refill || !dda || nr < 1 || nd < 1 || !chosen) return fail(AVR_ERR_ARG, "null argument");
    if (!c->has_medium || !c->has_film || !c->has_camera) return fail(AVR_ERR_STATE, "scene incomplete");
    if (spp_end <= spp_begin) return fail(AVR_ERR_ARG, "empty probe sample range");
    for (int k = 0; k < nr; ++k)
        if (refill[k] < 0 || refill[k] > 64) return fail(AVR_ERR_ARG, "refill candidates must be 0..64 lanes");
    for (int k = 0; k < nd; ++k)
        if (dda[k] < 0) return fail(AVR_ERR_ARG, "DDA budget candidates must be >= 0 cells");
    const int r0 = c->refill_min, d0 = c->dda_budget;
    // the default schedule (0, 0) when listed, else the current one, wins ties within the noise
    int prefer = -1;
    for (int k = 0; k < nr * nd && prefer < 0; ++k)
        if (refill[k / nd] == 0 && dda[k % nd] == 0) prefer = k;
    for (int k = 0; k < nr * nd && prefer < 0; ++k)
        if (refill[k / nd] == r0 && dda[k % nd] == d0) prefer = k;
    // every candidate that resolves to the preferred schedule counts as the same probe
    std::vector<char> same((size_t)nr * nd, 0);
    if (prefer >= 0) {
        int rp, dp;
        walk_schedule(c, refill[prefer / nd], dda[prefer % nd], &rp, &dp);
        for (int k = 0; k < nr * nd; ++k) {
            int rk, dk;
            walk_schedule(c, refill[k / nd], dda[k % nd], &rk, &dk);
            same[(size_t)k] = rk == rp && dk == dp;
        }
    }
    int bestk = 0;
    const int rc = probe_loop(
        c, nr * nd,
        [&](int k) {
            c->refill_min = refill[k / nd];
            c->dda_budget = dda[k % nd];
            return AVR_OK;
        },
        [&](bool failed, int b) {
            c->refill_min = failed ? r0 : refill[b / nd];
            c->dda_budget = failed ? d0 : dda[b % nd];
            return AVR_OK;
        },
        spp_begin, spp_end, seed, max_depth, &bestk, ms, prefer, &same);
    if (!rc) {
        chosen[0] = refill[bestk / nd];
        chosen[1] = dda[bestk % nd];
    }
    return rc;
}

static void pc1d_build(const float *f, int n, float mn, float mx, float *cdf, float *funcInt);

// ---------------------------------------------------------------------------
// PowerLightSampler (lightsamplers.cpp:76-96): weight = Average(SafeDiv(Phi(lambda),
// lambda.PDF())) at lambda = SampledWavelengths::SampleVisible(0.5) (canonical wavelength
// math, as the device's), then an AliasTable over the weights (util/sampling.cpp:563-618).
static avr::Spec visible_half_lambda(avr::Spec *pdf) {
    const avr::Spec l = avr::sample_visible_lambda(0.5f);
    *pdf = {avr::visible_wavelength_pdf(l.v0), avr::visible_wavelength_pdf(l.v1), avr::visible_wavelength_pdf(l.v2),
            avr::visible_wavelength_pdf(l.v3)};
    return l;
}
static float phi_weight(const avr::Spec &phi, const avr::Spec &pdf) {
    // SafeDiv then SampledSpectrum::Average (spectrum.h:175-181): sum in order, / 4
    const float a = pdf.v0 != 0 ? phi.v0 / pdf.v0 : 0.f, b = pdf.v1 != 0 ? phi.v1 / pdf.v1 : 0.f;
    const float c2 = pdf.v2 != 0 ? phi.v2 / pdf.v2 : 0.f, d = pdf.v3 != 0 ? phi.v3 / pdf.v3 : 0.f;
    return (((a + b) + c2) + d) / 4;
}
// DistantLight::Phi (lights.cpp:216-218): scale * Lemit(lambda) * Pi * Sqr(sceneRadius);
// UniformInfiniteLight::Phi (lights.cpp:974-976): 4 * Pi * Pi * Sqr(sceneRadius) * scale * Lemit(lambda)
static float phi_table_light(int type, const float *L, float scale, float r) {
    avr::Spec pdf;
    const avr::Spec l = visible_half_lambda(&pdf);
    const avr::Spec Le = avr::sample_table(L, avr::lambda_index(l));
    avr::Spec phi;
    if (type == 0) {
        phi = Le * scale * avr::kPi * (r * r);
    } else {
        const float k = 4 * avr::kPi * avr::kPi * (r * r) * scale;
        phi = avr::Spec{k * Le.v0, k * Le.v1, k * Le.v2, k * Le.v3};
    }
    return phi_weight(phi, pdf);
}
// PointLight::Phi (lights.cpp:164-166): 4 * Pi * scale * I(lambda); SpotLight::Phi
// (lights.cpp:1365-1368): scale * I(lambda) * 2 * Pi * ((1 - cosStart) + (cosStart - cosEnd) / 2)
static float phi_local_light(int type, const float *I, float scale, float cosStart, float cosEnd) {
    avr::Spec pdf;
    const avr::Spec l = visible_half_lambda(&pdf);
    const avr::Spec Il = avr::sample_table(I, avr::lambda_index(l));
    avr::Spec phi;
    if (type == avr::ll::kPoint) {
        const float k = 4 * avr::kPi * scale;
        phi = avr::Spec{k * Il.v0, k * Il.v1, k * Il.v2, k * Il.v3};
    } else {
        phi = Il * scale * 2.f * avr::kPi * ((1 - cosStart) + (cosStart - cosEnd) / 2);
    }
    return phi_weight(phi, pdf);
}
// RGBSigmoidPolynomial (util/color.h:332-365), the host twin of the device's rsp_eval
static float rsp_host(float c0, float c1, float c2, float lambda) {
    const float x = std::fma(lambda, std::fma(lambda, c0, c1), c2);
    if (std::isinf(x)) return x > 0 ? 1.f : 0.f;
    return .5f + x / (2 * std::sqrt(1 + x * x));
}
// ImageInfiniteLight::Phi (lights.cpp:1042-1060): the image's RGBIlluminantSpectrum summed over
// the pixels (rows y, then x) at lambda, times 4 Pi^2 R^2 scale / (width * height)
static float phi_image_light(const float *coeffs, int res, const float *illum, float scale, float r) {
    avr::Spec pdf;
    const avr::Spec l = visible_half_lambda(&pdf);
    const avr::Spec il = avr::sample_table(illum, avr::lambda_index(l));
    avr::Spec sum = avr::Spec::c(0.f);
    for (size_t p = 0; p < (size_t)res * res; ++p) {
        const float *c = coeffs + 4 * p;
        const avr::Spec s{c[3] * rsp_host(c[0], c[1], c[2], l.v0), c[3] * rsp_host(c[0], c[1], c[2], l.v1),
                          c[3] * rsp_host(c[0], c[1], c[2], l.v2), c[3] * rsp_host(c[0], c[1], c[2], l.v3)};
        sum = sum + s * il;
    }
    const float k = 4 * avr::kPi * avr::kPi * (r * r) * scale;
    const float wh = (float)(res * res);
    const avr::Spec phi{k * sum.v0 / wh, k * sum.v1 / wh, k * sum.v2 / wh, k * sum.v3 / wh};
    return phi_weight(phi, pdf);
}
// AliasTable construction (util/sampling.cpp:563-618): p = w / sum (double accumulation),
// then the under / over work lists popped from the back
static void build_alias(const float *w, int n, float *q, float *p, int *alias) {
    double acc = 0.;
    for (int i = 0; i < n; ++i) acc += w[i];
    const float sum = (float)acc;
    for (int i = 0; i < n; ++i) p[i] = w[i] / sum;
    struct Outcome { float pHat; int index; };
    std::vector<Outcome> under, over;
    for (int i = 0; i < n; ++i) {
        const float pHat = p[i] * (float)n;
        (pHat < 1 ? under : over).push_back({pHat, i});
    }
    while (!under.empty() && !over.empty()) {
        const Outcome un = under.back(), ov = over.back();
        under.pop_back();
        over.pop_back();
        q[un.index] = un.pHat;
        alias[un.index] = ov.index;
        const float pExcess = un.pHat + ov.pHat - 1;
        (pExcess < 1 ? under : over).push_back({pExcess, ov.index});
    }
    for (const Outcome &o : over) q[o.index] = 1, alias[o.index] = -1;
    for (const Outcome &u : under) q[u.index] = 1, alias[u.index] = -1;
}
// (Re)build the device light list's sampler fields after any light or sampler change
static int update_light_sampler(avr_context *c) {
    const int n = c->lights.n;
    bool ready = c->light_sampler == 1 && n > 0;
    for (int i = 0; i < n && ready; ++i) ready = c->phi_ok[i];
    // lists of infinite lights: "bvh" and "uniform" are the one pick every kernel evaluates; with
    // a local light, BVHLightSampler's traversal or UniformLightSampler over the whole list
    const int plain = c->n_local_lights == 0 ? avr::kPickInfinite
                                             : (c->light_sampler == 2 ? avr::kPickUniform : avr::kPickBvh);
    c->lights.mode = ready ? avr::kPickPower : plain;
    if (n == 0) return AVR_OK;
    // BVHLightSampler's constructor over the list, once every local light has its transform
    bool localReady = c->n_local_lights > 0;
    for (int i = 0; i < n && localReady; ++i) localReady = c->h_lights[i].type < avr::ll::kPoint || c->local_ok[i];
    c->h_tree = avr::ll::Tree{};
    if (localReady) {
        bool bounded[avr::kMaxLights] = {};
        avr::ll::LightBounds lb[avr::kMaxLights];
        for (int i = 0; i < n; ++i) {
            const avr::DevLight &L = c->h_lights[i];
            bounded[i] = L.type >= avr::ll::kPoint;
            if (!bounded[i]) continue;
            const float *I = c->h_lightL.data() + (size_t)i * avr::kNTable;
            const float maxI = *std::max_element(I, I + avr::kNTable);   // DenselySampledSpectrum::MaxValue
            lb[i] = avr::ll::light_bounds(L.type, c->h_rfl[i], L.scale, maxI, L.cos_start, L.cos_end);
        }
        avr::ll::build_tree(n, bounded, lb, &c->h_tree);
    }
    if (c->d_lights) {
        HIP_TRY(hipMemcpyAsync(c->d_lights.get() + avr::kMaxLights, &c->h_tree, sizeof(c->h_tree), hipMemcpyHostToDevice,
                               c->stream));
    }
    float q[avr::kMaxLights], pm[avr::kMaxLights];
    int al[avr::kMaxLights];
    if (ready) {
        float w[avr::kMaxLights];
        float tot = 0.f;
        for (int i = 0; i < n; ++i) tot += (w[i] = c->h_phi[i]);   // std::accumulate(..., 0.f)
        if (tot == 0.f) std::fill(w, w + n, 1.f);
        build_alias(w, n, q, pm, al);
    } else {
        // BVH / uniform (the kernels' pick ignores the bins then): q = 1, p = pInf / n
        for (int i = 0; i < n; ++i) q[i] = 1.f, pm[i] = float(n) / float(n + 0) / n, al[i] = -1;
    }
    for (int i = 0; i < n; ++i) {
        c->h_lights[i].aq = q[i];
        c->h_lights[i].ap = pm[i];
        c->h_lights[i].alias = al[i];
    }
    if (c->d_lights) {
        HIP_TRY(hipMemcpyAsync(c->d_lights.get(), c->h_lights, sizeof(c->h_lights), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return AVR_OK;
}

int avr_lights(avr_context *c, int n, const int *types, const float *w3, const float *L, const float *scale,
               float scene_radius) {
    AVR_QUIESCE(c);
    if (!c || n < 0 || n > avr::kMaxLights) return fail(AVR_ERR_ARG, "0..8 lights supported");
    if (n > 0 && (!types || !w3 || !L || !scale)) return fail(AVR_ERR_ARG, "null light arrays");
    HIP_TRY(hipSetDevice(c->device));
    int rc = upload_table(c->d_lightL, n ? L : nullptr, (size_t)n * avr::kNTable, c->stream);
    if (rc) return rc;
    avr::DevLight h[avr::kMaxLights] = {};
    for (int i = 0; i < n; ++i) {
        if (types[i] < 0 || types[i] > 4)
            return fail(AVR_ERR_ARG, "light type must be 0 (distant), 1 (uniform infinite), 2 (image infinite), "
                                     "3 (point) or 4 (spot)");
        h[i].type = types[i];
        for (int k = 0; k < 3; ++k) h[i].w[k] = w3[3 * i + k];
        h[i].L = c->d_lightL.get() + (size_t)i * avr::kNTable;
        h[i].scale = scale[i];
    }
    // (the records, and behind them the light BVH: light_tree())
    if (!c->d_lights) HIP_TRY(c->d_lights.alloc(avr::kMaxLights + avr::kLightTreeSlots));
    HIP_TRY(hipMemcpyAsync(c->d_lights.get(), h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (auto &b : c->d_light_img) b.reset();
    for (int i = 0; i < avr::kMaxLights; ++i) c->h_lights[i] = h[i];
    c->lights = {};
    c->lights.n = n;
    c->lights.list = c->d_lights.get();
    c->lights.scene_radius = scene_radius;
    c->n_image_lights = 0;
    c->n_local_lights = 0;
    for (int i = 0; i < n; ++i) c->n_image_lights += types[i] == 2 ? 1 : 0;
    for (int i = 0; i < n; ++i) c->n_local_lights += types[i] >= avr::ll::kPoint ? 1 : 0;
    c->h_lightL.assign(L, L + (size_t)n * avr::kNTable);
    for (int i = 0; i < avr::kMaxLights; ++i) {
        c->local_ok[i] = false;
        // an image light's Phi needs its image, a local light's its cone (avr_light_local)
        c->phi_ok[i] = i < n && types[i] < 2;
        c->h_phi[i] = c->phi_ok[i] ? phi_table_light(types[i], L + (size_t)i * avr::kNTable, scale[i], scene_radius) : 0.f;
    }
    return update_light_sampler(c);
}

int avr_light_sampler(avr_context *c, int kind) {
    AVR_QUIESCE(c);
    if (!c || kind < 0 || kind > 2) return fail(AVR_ERR_ARG, "light sampler must be 0 (bvh), 1 (power) or 2 (uniform)");
    HIP_TRY(hipSetDevice(c->device));
    c->light_sampler = kind;
    return update_light_sampler(c);
}

// ImageInfiniteLight: pixel spectra, the compensated PiecewiseConstant2D (lights.cpp:1026-1038)
int avr_light_image(avr_context *c, int index, int res, const float *pixel_coeffs, const float *distribution,
                    const float *illuminant, const float render_from_light[16], const float light_from_render[16]) {
    AVR_QUIESCE(c);
    if (!c || index < 0 || index >= c->lights.n || c->h_lights[index].type != 2)
        return fail(AVR_ERR_ARG, "avr_light_image: index must name a type-2 light of the last avr_lights call");
    if (res < 1 || !pixel_coeffs || !distribution || !illuminant || !render_from_light || !light_from_render)
        return fail(AVR_ERR_ARG, "avr_light_image: bad image arguments");
    HIP_TRY(hipSetDevice(c->device));
    const size_t np = (size_t)res * res;
    // compensated distribution: d - average (f64 accumulate, lights.cpp:1031), clamped at 0;
    // all zero -> ones
    double sum = 0.;
    for (size_t i = 0; i < np; ++i) sum += distribution[i];
    const float average = (float)(sum / np);
    std::vector<float> d(np);
    bool allZero = true;
    for (size_t i = 0; i < np; ++i) {
        d[i] = std::max<float>(distribution[i] - average, 0);
        allZero &= d[i] == 0;
    }
    if (allZero) std::fill(d.begin(), d.end(), 1.f);
    const int nx = res, ny = res;
    const size_t ntab = (size_t)avr::smp::filter_table_floats(nx, ny);
    const size_t bytes = np * sizeof(float4) + ntab * sizeof(float) + avr::kNTable * sizeof(float);
    std::vector<unsigned char> blob(bytes);
    std::memcpy(blob.data(), pixel_coeffs, np * sizeof(float4));
    float *t = (float *)(blob.data() + np * sizeof(float4));
    float *f = t, *ccdf = f + nx * ny, *cint = ccdf + ny * (nx + 1), *mcdf = cint + ny, *mint = mcdf + ny + 1;
    for (size_t i = 0; i < np; ++i) f[i] = std::abs(d[i]);
    for (int y = 0; y < ny; ++y) pc1d_build(f + (size_t)y * nx, nx, 0.f, 1.f, ccdf + (size_t)y * (nx + 1), cint + y);
    pc1d_build(cint, ny, 0.f, 1.f, mcdf, mint);
    std::memcpy(t + ntab, illuminant, avr::kNTable * sizeof(float));
    HIP_TRY(c->d_light_img[index].alloc(bytes));
    unsigned char *base = c->d_light_img[index].get();
    HIP_TRY(hipMemcpy(base, blob.data(), bytes, hipMemcpyHostToDevice));
    avr::DevLight &L = c->h_lights[index];
    L.img = (const float4 *)base;
    L.res = res;
    const float *dt = (const float *)(base + np * sizeof(float4));
    L.dist.nx = nx;
    L.dist.ny = ny;
    L.dist.f = dt;
    L.dist.ccdf = dt + nx * ny;
    L.dist.cint = L.dist.ccdf + ny * (nx + 1);
    L.dist.mcdf = L.dist.cint + ny;
    L.dist.mint = *mint;
    L.illum = dt + ntab;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            L.rfl[3 * r + k] = render_from_light[4 * r + k];
            L.lfr[3 * r + k] = light_from_render[4 * r + k];
        }
    HIP_TRY(hipMemcpyAsync(c->d_lights.get(), c->h_lights, sizeof(c->h_lights), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->h_phi[index] = phi_image_light(pixel_coeffs, res, illuminant, L.scale, c->lights.scene_radius);
    c->phi_ok[index] = true;
    return update_light_sampler(c);
}

// PointLight / SpotLight: the transforms and the cone of a type-3 / type-4 light
int avr_light_local(avr_context *c, int index, const float render_from_light[16], const float light_from_render[16],
                    float cos_falloff_start, float cos_falloff_end) {
    AVR_QUIESCE(c);
    if (!c || index < 0 || index >= c->lights.n || c->h_lights[index].type < avr::ll::kPoint)
        return fail(AVR_ERR_ARG, "avr_light_local: index must name a type-3 or type-4 light of the last avr_lights call");
    if (!render_from_light || !light_from_render) return fail(AVR_ERR_ARG, "avr_light_local: null transform");
    HIP_TRY(hipSetDevice(c->device));
    avr::DevLight &L = c->h_lights[index];
    for (int i = 0; i < 16; ++i) c->h_rfl[index][i] = render_from_light[i];
    avr::ll::light_position(render_from_light, L.w);
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            L.rfl[3 * r + k] = render_from_light[4 * r + k];
            L.lfr[3 * r + k] = light_from_render[4 * r + k];
        }
    L.cos_start = cos_falloff_start;
    L.cos_end = cos_falloff_end;
    c->local_ok[index] = true;
    c->h_phi[index] = phi_local_light(L.type, c->h_lightL.data() + (size_t)index * avr::kNTable, L.scale, L.cos_start,
                                      L.cos_end);
    c->phi_ok[index] = true;
    return update_light_sampler(c);
}

// Whether every type-2 light of the list has its image (avr_light_image)
static bool image_lights_complete(const avr_context *c) {
    for (int i = 0; i < c->lights.n; ++i)
        if (c->h_lights[i].type == 2 && !c->d_light_img[i]) return false;
    return true;
}
// Whether every type-3 / type-4 light of the list has its transform (avr_light_local)
static bool local_lights_complete(const avr_context *c) {
    for (int i = 0; i < c->lights.n; ++i)
        if (c->h_lights[i].type >= avr::ll::kPoint && !c->local_ok[i]) return false;
    return true;
}

int avr_light_probe(avr_context *c, int index, int n, const float *u2, const float *w3, const float *lambda4,
                    float *wi3, float *pdf_sample, float *Ls4, float *pdf_li, float *Le4) {
    AVR_QUIESCE(c);
    if (!c || index < 0 || index >= c->lights.n) return fail(AVR_ERR_ARG, "avr_light_probe: index must name a light");
    if (n < 0 || n > 1 << 20 || (n > 0 && (!u2 || !w3 || !lambda4))) return fail(AVR_ERR_ARG, "avr_light_probe: bad probe arrays");
    if (!image_lights_complete(c)) return fail(AVR_ERR_STATE, "image light without avr_light_image");
    if (!local_lights_complete(c)) return fail(AVR_ERR_STATE, "point or spot light without avr_light_local");
    if (n == 0) return AVR_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t N = (size_t)n;
    Arena<> scratch(c->stream);
    const auto ru = scratch.reserve<float>(2 * N), rw = scratch.reserve<float>(3 * N), rl = scratch.reserve<float>(4 * N);
    const auto rwi = scratch.reserve<float>(3 * N), rps = scratch.reserve<float>(N), rLs = scratch.reserve<float>(4 * N);
    const auto rpl = scratch.reserve<float>(N), rLe = scratch.reserve<float>(4 * N);
    HIP_TRY(scratch.commit());
    float *du = scratch.get(ru), *dw = scratch.get(rw), *dl = scratch.get(rl), *dwi = scratch.get(rwi);
    float *dps = scratch.get(rps), *dLs = scratch.get(rLs), *dpl = scratch.get(rpl), *dLe = scratch.get(rLe);
    HIP_TRY(hipMemcpyAsync(du, u2, 2 * N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dw, w3, 3 * N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dl, lambda4, 4 * N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(avr::k_light_probe, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->lights, index, n, du, dw, dl,
                       dwi, dps, dLs, dpl, dLe);
    HIP_TRY(hipGetLastError());
    const struct { float *host; const float *dev; size_t k; } outs[] = {{wi3, dwi, 3}, {pdf_sample, dps, 1}, {Ls4, dLs, 4},
                                                                       {pdf_li, dpl, 1}, {Le4, dLe, 4}};
    for (const auto &o : outs)
        if (o.host) HIP_TRY(hipMemcpyAsync(o.host, o.dev, o.k * N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

// avr_light_pick (p3 null: the origin) and avr_light_pick_at
static int light_pick_impl(avr_context *c, int n, const float *u, const float *p3, int *idx, float *pmf) {
    if (c->light_sampler == 1 && c->lights.n > 0 && c->lights.mode != avr::kPickPower)
        return fail(AVR_ERR_STATE, "power light sampler: light weights incomplete");
    if (!local_lights_complete(c)) return fail(AVR_ERR_STATE, "point or spot light without avr_light_local");
    if (n == 0) return AVR_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t N = (size_t)n;
    Arena<> scratch(c->stream);
    const auto ru = scratch.reserve<float>(N), rp = scratch.reserve<float>(N), rpt = scratch.reserve<float>(3 * N);
    const auto ri = scratch.reserve<int>(N);
    HIP_TRY(scratch.commit());
    float *du = scratch.get(ru), *dp = scratch.get(rp), *dpt = scratch.get(rpt);
    int *di = scratch.get(ri);
    HIP_TRY(hipMemcpyAsync(du, u, N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (p3) HIP_TRY(hipMemcpyAsync(dpt, p3, 3 * N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(avr::k_light_pick, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->lights, n, du,
                       p3 ? dpt : nullptr, di, dp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(idx, di, N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(pmf, dp, N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}
int avr_light_pick(avr_context *c, int n, const float *u, int *idx, float *pmf) {
    AVR_QUIESCE(c);
    if (!c || n < 0 || n > 1 << 20 || (n > 0 && (!u || !idx || !pmf))) return fail(AVR_ERR_ARG, "avr_light_pick: bad arrays");
    return light_pick_impl(c, n, u, nullptr, idx, pmf);
}
int avr_light_pick_at(avr_context *c, int n, const float *u, const float *p3, int *idx, float *pmf) {
    AVR_QUIESCE(c);
    if (!c || n < 0 || n > 1 << 20 || (n > 0 && (!u || !p3 || !idx || !pmf)))
        return fail(AVR_ERR_ARG, "avr_light_pick_at: bad arrays");
    return light_pick_impl(c, n, u, p3, idx, pmf);
}

int avr_light_probe_at(avr_context *c, int index, int n, const float *u2, const float *p3, const float *lambda4,
                       float *wi3, float *pdf_sample, float *Ls4, float *dist) {
    AVR_QUIESCE(c);
    if (!c || index < 0 || index >= c->lights.n) return fail(AVR_ERR_ARG, "avr_light_probe_at: index must name a light");
    if (n < 0 || n > 1 << 20 || (n > 0 && (!u2 || !p3 || !lambda4)))
        return fail(AVR_ERR_ARG, "avr_light_probe_at: bad probe arrays");
    if (!image_lights_complete(c)) return fail(AVR_ERR_STATE, "image light without avr_light_image");
    if (!local_lights_complete(c)) return fail(AVR_ERR_STATE, "point or spot light without avr_light_local");
    if (n == 0) return AVR_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t N = (size_t)n;
    Arena<> scratch(c->stream);
    const auto ru = scratch.reserve<float>(2 * N), rp = scratch.reserve<float>(3 * N), rl = scratch.reserve<float>(4 * N);
    const auto rwi = scratch.reserve<float>(3 * N), rps = scratch.reserve<float>(N), rLs = scratch.reserve<float>(4 * N);
    const auto rr = scratch.reserve<float>(N);
    HIP_TRY(scratch.commit());
    float *du = scratch.get(ru), *dp = scratch.get(rp), *dl = scratch.get(rl), *dwi = scratch.get(rwi);
    float *dps = scratch.get(rps), *dLs = scratch.get(rLs), *dr = scratch.get(rr);
    HIP_TRY(hipMemcpyAsync(du, u2, 2 * N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dp, p3, 3 * N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dl, lambda4, 4 * N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(avr::k_light_probe_at, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->lights, index, n, du, dp,
                       dl, dwi, dps, dLs, dr);
    HIP_TRY(hipGetLastError());
    const struct { float *host; const float *dev; size_t k; } outs[] = {{wi3, dwi, 3}, {pdf_sample, dps, 1}, {Ls4, dLs, 4},
                                                                       {dist, dr, 1}};
    for (const auto &o : outs)
        if (o.host) HIP_TRY(hipMemcpyAsync(o.host, o.dev, o.k * N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_light_bvh(avr_context *c, int *n_nodes, float *phi, float *w3, int *qcos, int *qb, int *link, int *leaf,
                  float all_bounds[6], int *n_infinite) {
    if (!c) return fail(AVR_ERR_ARG, "avr_light_bvh: null context");
    if (!local_lights_complete(c)) return fail(AVR_ERR_STATE, "point or spot light without avr_light_local");
    const avr::ll::Tree &t = c->h_tree;
    if (n_nodes) *n_nodes = t.nNodes;
    if (n_infinite) *n_infinite = c->n_local_lights > 0 ? t.nInf : c->lights.n;
    for (int i = 0; i < t.nNodes; ++i) {
        const avr::ll::Node &nd = t.nodes[i];
        if (phi) phi[i] = nd.phi;
        if (w3) avr::ll::oct_decode(nd.wx, nd.wy, w3 + 3 * i);
        if (qcos) qcos[2 * i] = (int)nd.q_cos_o(), qcos[2 * i + 1] = (int)nd.q_cos_e();
        if (qb)
            for (int k = 0; k < 6; ++k) qb[6 * i + k] = nd.qb[k / 3][k % 3];
        if (link) link[i] = (int)nd.index();
        if (leaf) leaf[i] = nd.leaf() ? 1 : 0;
    }
    if (all_bounds)
        for (int k = 0; k < 6; ++k) all_bounds[k] = t.allb[k];
    return AVR_OK;
}

int avr_light_sampler_table(avr_context *c, float *q, float *p, int *alias) {
    if (!c || (c->lights.n > 0 && (!q || !p || !alias))) return fail(AVR_ERR_ARG, "avr_light_sampler_table: null arg");
    if (c->light_sampler == 1 && c->lights.n > 0 && c->lights.mode != avr::kPickPower)
        return fail(AVR_ERR_STATE, "power light sampler: light weights incomplete");
    for (int i = 0; i < c->lights.n; ++i) {
        q[i] = c->h_lights[i].aq;
        p[i] = c->h_lights[i].ap;
        alias[i] = c->h_lights[i].alias;
    }
    return AVR_OK;
}

int avr_camera(avr_context *c, int type, const float cfr[16], const float rfc[16]) {
    if (!c || (type != 0 && type != 1) || !cfr || !rfc) return fail(AVR_ERR_ARG, "bad camera");
    if (!affine(rfc)) return fail(AVR_ERR_ARG, "render_from_camera must be affine");
    c->cam.type = type;
    for (int i = 0; i < 16; ++i) c->cam.raster[i] = cfr[i];
    copy_xf(c->cam.render_from_camera, rfc);
    c->cam.lens_radius = 0.f;   // the pinhole (avr_camera_lens sets a lens)
    c->cam.focal_distance = 1e6f;
    c->cam.mapping = 0;
    c->has_camera = true;
    return AVR_OK;
}

int avr_camera_lens(avr_context *c, float lens_radius, float focal_distance) {
    if (!c) return fail(AVR_ERR_ARG, "null context");
    if (!(lens_radius >= 0.f) || !std::isfinite(lens_radius)) return fail(AVR_ERR_ARG, "lens radius must be finite and >= 0");
    if (!(focal_distance > 0.f)) return fail(AVR_ERR_ARG, "focal distance must be > 0");
    if (!c->has_camera) return fail(AVR_ERR_STATE, "the lens needs a camera (avr_camera first)");
    if (c->cam.type == avr::cam::kSpherical) return fail(AVR_ERR_ARG, "a spherical camera has no lens");
    AVR_QUIESCE(c);   // camera records made ahead for the old lens are dropped
    c->cam.lens_radius = lens_radius;
    c->cam.focal_distance = focal_distance;
    return AVR_OK;
}

int avr_camera_spherical(avr_context *c, int mapping, const float rfc[16]) {
    if (!c || (mapping != avr::cam::kEqualArea && mapping != avr::cam::kEquiRectangular) || !rfc)
        return fail(AVR_ERR_ARG, "bad spherical camera (mapping: 0 equalarea, 1 equirectangular)");
    if (!affine(rfc)) return fail(AVR_ERR_ARG, "render_from_camera must be affine");
    AVR_QUIESCE(c);   // camera records made ahead for the old camera are dropped
    c->cam.type = avr::cam::kSpherical;
    for (int i = 0; i < 16; ++i) c->cam.raster[i] = (i % 5 == 0) ? 1.f : 0.f;   // unused: pFilm maps directly
    copy_xf(c->cam.render_from_camera, rfc);
    c->cam.lens_radius = 0.f;
    c->cam.focal_distance = 1e6f;
    c->cam.mapping = mapping;
    c->has_camera = true;
    return AVR_OK;
}

int avr_film(avr_context *c, int width, int height, const float fr[2], const float *sensor, float imaging_ratio,
             float max_component_value) {
    AVR_QUIESCE(c);
    if (!c || width < 1 || height < 1 || !fr || !sensor) return fail(AVR_ERR_ARG, "bad film");
    HIP_TRY(hipSetDevice(c->device));
    int rc = upload_table(c->d_xyz, sensor, 3 * (size_t)avr::kNTable, c->stream);
    if (rc) return rc;
    free_film_sums(c);
    free_pixel_order(c);   // an order is for one film resolution
    c->d_aacc.reset();     // the analysis' per-pixel sums go with the film
    c->last.analyze = 0;
    c->film = {};
    c->film.width = width;
    c->film.height = height;
    c->film.bw = width;   // the bounds: the whole film (avr_film_pixel_bounds)
    c->film.bh = height;
    c->film.filter_rx = fr[0];
    c->film.filter_ry = fr[1];
    c->film.xyz = c->d_xyz.get();
    c->film.imaging_ratio = imaging_ratio;
    c->film.max_component = max_component_value;
    if ((rc = alloc_film_sums(c))) return rc;
    c->has_film = true;
    return avr_film_clear(c);
}

// Film::pixelBounds (film.h:67, film.cpp:97-172): the film's sums, readbacks and per-sample
// records shrink to [x0, x1) x [y0, y1); samplers and the camera keep the full resolution, so
// the bounds' pixels get the samples they get in a render of the whole film.
int avr_film_pixel_bounds(avr_context *c, int x0, int y0, int x1, int y1) {
    AVR_QUIESCE(c);
    if (!c || !c->has_film) return fail(AVR_ERR_STATE, "pixel bounds need a film (avr_film first)");
    if (x0 >= x1 || y0 >= y1) return fail(AVR_ERR_ARG, "pixel bounds are empty");
    if (x0 < 0 || y0 < 0 || x1 > c->film.width || y1 > c->film.height)
        return fail(AVR_ERR_ARG, "pixel bounds [" + std::to_string(x0) + ", " + std::to_string(x1) + ") x [" +
                                     std::to_string(y0) + ", " + std::to_string(y1) + ") reach outside the " +
                                     std::to_string(c->film.width) + " x " + std::to_string(c->film.height) + " film");
    HIP_TRY(hipSetDevice(c->device));
    // what was made for the old bounds: the pixel order, the analysis sums, the metric reference,
    // the ZSobol pixel and level-A tables, and the pass table and camera records built ahead
    free_pixel_order(c);
    c->d_aacc.reset();
    c->last = LastPass{};
    c->d_reference.reset();
    c->d_image.reset();
    c->look.invalidate();
    c->zs_key[0] = -1;
    for (long long &k : c->zs_akey) k = -1;
    free_film_sums(c);
    c->film.x0 = x0;
    c->film.y0 = y0;
    c->film.bw = x1 - x0;
    c->film.bh = y1 - y0;
    const int rc = alloc_film_sums(c);
    return rc ? rc : avr_film_clear(c);
}

int avr_film_get_bounds(avr_context *c, int *x0, int *y0, int *x1, int *y1) {
    if (!c || !c->has_film || !x0 || !y0 || !x1 || !y1) return fail(AVR_ERR_STATE, "no film or null argument");
    *x0 = c->film.x0;
    *y0 = c->film.y0;
    *x1 = c->film.x0 + c->film.bw;
    *y1 = c->film.y0 + c->film.bh;
    return AVR_OK;
}

// FilterSampler tables of GaussianFilter(radius, sigma) — filters.h:80-118,
// filters.cpp:133-147, PiecewiseConstant1D/2D sampling.h:603-770 — built on the host in
// pbrt's float operation order (this file is compiled with -ffp-contract=off).
static float gaussian_1d(float x, float mu, float sigma) {   // util/math.h:477-480
    return 1 / std::sqrt(2 * avr::kPi * sigma * sigma) * avr::fast_exp(-avr::sqr(x - mu) / (2 * sigma * sigma));
}
static void pc1d_build(const float *f, int n, float mn, float mx, float *cdf, float *funcInt) {
    cdf[0] = 0;
    for (int i = 1; i < n + 1; ++i) cdf[i] = cdf[i - 1] + std::abs(f[i - 1]) * (mx - mn) / n;
    *funcInt = cdf[n];
    if (*funcInt == 0)
        for (int i = 1; i < n + 1; ++i) cdf[i] = float(i) / float(n);
    else
        for (int i = 1; i < n + 1; ++i) cdf[i] /= *funcInt;
}

int avr_set_filter(avr_context *c, int type, const float radius[2], float sigma) {
    AVR_QUIESCE(c);
    if (!c || (type != 0 && type != 1) || !radius || !(radius[0] > 0) || !(radius[1] > 0))
        return fail(AVR_ERR_ARG, "filter: type 0 (box) or 1 (gaussian) with a positive radius");
    HIP_TRY(hipSetDevice(c->device));
    if (type == 0) {
        c->filter_type = 0;
        c->film.filter_rx = radius[0];
        c->film.filter_ry = radius[1];
        return AVR_OK;
    }
    const int nx = int(32 * radius[0]), ny = int(32 * radius[1]);
    if (nx < 1 || ny < 1 || nx > 128 || ny > 128) return fail(AVR_ERR_ARG, "gaussian filter radius out of range");
    const float expX = gaussian_1d(radius[0], 0, sigma), expY = gaussian_1d(radius[1], 0, sigma);
    std::vector<float> t((size_t)avr::smp::filter_table_floats(nx, ny));
    float *f = t.data(), *ccdf = f + nx * ny, *cint = ccdf + ny * (nx + 1), *mcdf = cint + ny, *mint = mcdf + ny + 1;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            // Bounds2f::Lerp of ((x + 0.5) / nx, (y + 0.5) / ny) over [-r, r]
            const float tx = (x + 0.5f) / nx, ty = (y + 0.5f) / ny;
            const float px = (1 - tx) * -radius[0] + tx * radius[0], py = (1 - ty) * -radius[1] + ty * radius[1];
            f[(size_t)y * nx + x] = std::max<float>(0, gaussian_1d(px, 0, sigma) - expX) *
                                    std::max<float>(0, gaussian_1d(py, 0, sigma) - expY);
        }
    for (int y = 0; y < ny; ++y) pc1d_build(f + (size_t)y * nx, nx, -radius[0], radius[0], ccdf + (size_t)y * (nx + 1), cint + y);
    pc1d_build(cint, ny, -radius[1], radius[1], mcdf, mint);
    // the search guides (camera stage): one row per conditional CDF, then the marginal's
    t.resize((size_t)avr::smp::filter_blob_floats(nx, ny), 0.f);
    f = t.data();
    ccdf = f + nx * ny;
    cint = ccdf + ny * (nx + 1);
    mcdf = cint + ny;
    const float mint_v = t[(size_t)avr::smp::filter_table_floats(nx, ny) - 1];
    uint8_t *guide = (uint8_t *)(t.data() + avr::smp::filter_table_floats(nx, ny));
    for (int y = 0; y < ny; ++y)
        avr::smp::filter_guide_build(ccdf + (size_t)y * (nx + 1), nx, guide + (size_t)y * (avr::smp::kFilterGuideK + 1));
    avr::smp::filter_guide_build(mcdf, ny, guide + (size_t)ny * (avr::smp::kFilterGuideK + 1));
    // the cell weights (after the guides)
    float *wt = t.data() + avr::smp::filter_table_floats(nx, ny) + avr::smp::filter_guide_floats(ny);
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) wt[(size_t)y * nx + x] = avr::smp::filter_cell_weight(f, cint, mint_v, nx, y, x);
    HIP_TRY(c->d_filter.alloc(t.size()));
    const float *d_filter = c->d_filter.get();
    HIP_TRY(hipMemcpy(c->d_filter.get(), t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    c->ftab.nx = nx;
    c->ftab.ny = ny;
    c->ftab.rx = radius[0];
    c->ftab.ry = radius[1];
    c->ftab.f = d_filter;
    c->ftab.ccdf = d_filter + nx * ny;
    c->ftab.cint = c->ftab.ccdf + ny * (nx + 1);
    c->ftab.mcdf = c->ftab.cint + ny;
    c->ftab.mint = mint_v;
    c->ftab.guide = (const uint8_t *)(d_filter + avr::smp::filter_table_floats(nx, ny));
    c->ftab.wt = d_filter + avr::smp::filter_table_floats(nx, ny) + avr::smp::filter_guide_floats(ny);
    c->filter_type = 1;
    return AVR_OK;
}

int avr_set_pixel_order(avr_context *c, const int *order, long long n) {
    AVR_QUIESCE(c);
    if (!c || !c->has_film) return fail(AVR_ERR_STATE, "pixel order needs a film");
    HIP_TRY(hipSetDevice(c->device));
    free_pixel_order(c);
    if (!order) return AVR_OK;   // scanline
    const long long np = (long long)c->film.bw * c->film.bh;
    if (n != np) return fail(AVR_ERR_ARG, "pixel order must list every pixel of the film once");
    std::vector<int> slot((size_t)np, -1);
    for (long long j = 0; j < np; ++j) {
        const int p = order[j];
        if (p < 0 || p >= np || slot[(size_t)p] >= 0) return fail(AVR_ERR_ARG, "pixel order is not a permutation");
        slot[(size_t)p] = (int)j;
    }
    HIP_TRY(c->d_pix_order.alloc((size_t)np));
    HIP_TRY(c->d_pix_slot.alloc((size_t)np));
    HIP_TRY(hipMemcpy(c->d_pix_order.get(), order, np * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_pix_slot.get(), slot.data(), np * sizeof(int), hipMemcpyHostToDevice));
    c->h_pix_slot.swap(slot);
    ++c->order_gen;
    return AVR_OK;
}

int avr_set_sampler_table(avr_context *c, int dims) {
    AVR_QUIESCE(c);
    if (!c || dims < 0 || dims > 4096) return fail(AVR_ERR_ARG, "sampler table dimensions must be 0..4096");
    c->zs_dims = dims;
    c->zs_key[0] = -1;   // rebuild (or drop) at the next render
    return AVR_OK;
}

int avr_set_sampler_pass_table(avr_context *c, int dims) {
    AVR_QUIESCE(c);
    if (!c || dims < 0 || dims > 4096) return fail(AVR_ERR_ARG, "sampler pass table dimensions must be 0..4096");
    // rows of an even number of 8-B entries: the camera stage loads a draw pair's entries as one
    // 16-B ulonglong2 at ptab + row * dims, aligned only for even dims (the extra dimension is
    // never read — same results)
    c->zs_pdims = (dims + 1) & ~1;
    return AVR_OK;
}

int avr_set_sampler(avr_context *c, int kind, int samples_per_pixel) {
    if (!c || (kind != 0 && kind != 1) || samples_per_pixel < 1)
        return fail(AVR_ERR_ARG, "sampler: kind 0 (independent) or 1 (zsobol), samples_per_pixel >= 1");
    c->sampler_kind = kind;
    c->sampler_spp = samples_per_pixel;
    return AVR_OK;
}

int avr_film_clear(avr_context *c) {
    if (!c || !c->has_film) return fail(AVR_ERR_STATE, "no film");
    const size_t np = (size_t)c->film.bw * c->film.bh;
    HIP_TRY(hipMemsetAsync(c->film.rgb_sum, 0, 3 * np * sizeof(double), c->stream));
    HIP_TRY(hipMemsetAsync(c->film.w_sum, 0, np * sizeof(double), c->stream));
    if (c->film.nbuckets > 0)
        HIP_TRY(hipMemsetAsync(c->film.bucket_sum, 0, 2 * np * c->film.nbuckets * sizeof(double), c->stream));
    return AVR_OK;
}

// SpectralFilm (film.h:401-530, Create film.cpp:1037-1066): buckets over [lambda_min,
// lambda_max]; n_buckets = 0 returns to RGBFilm. Both sums live in one allocation.
int avr_film_spectral(avr_context *c, int n_buckets, float lambda_min, float lambda_max) {
    if (!c || !c->has_film) return fail(AVR_ERR_STATE, "no film");
    if (n_buckets < 0) return fail(AVR_ERR_ARG, "n_buckets must be >= 0");
    if (n_buckets > 0 && !(360.f <= lambda_min && lambda_min < lambda_max && lambda_max <= 830.f))
        return fail(AVR_ERR_ARG, "SpectralFilm wavelength range must lie within 360..830 nm");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->d_film_bucket.reset();
    c->film.bucket_sum = c->film.bucket_w = nullptr;
    c->film.nbuckets = n_buckets;
    c->film.lmin = lambda_min;
    c->film.lmax = lambda_max;
    const int rc = alloc_film_sums(c);   // (the rgb and weight sums stay: the bucket sums only)
    return rc ? rc : avr_film_clear(c);
}

// Stats are resolved lazily so that a render stays asynchronous: every timed interval
// records two pool events and is folded (one stream sync) when stats are read.
static int fold_stats(avr_context *c) {
    if (c->timed.empty()) return AVR_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->tstream) HIP_TRY(hipStreamSynchronize(c->tstream));   // (a camera stage run ahead is timed there)
    for (const auto &t : c->timed) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->evpool[t.a], c->evpool[t.b]));
        c->stats.*(t.field) += ms;
        if (t.launch) c->stats.medium_launches++;
    }
    c->timed.clear();
    c->ev_used = 0;
    unsigned long long h[avr::kNumStats];
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(h, c->d_stats.get(), sizeof(h), hipMemcpyDeviceToHost));
    c->stats.medium_lookups = h[0];
    c->stats.medium_items_in = h[1];
    c->stats.medium_items_out = h[2];
    c->stats.shadow_lookups = h[3];
    c->stats.shadow_items = h[4];
    c->stats.medium_dda_steps = h[5];
    c->stats.shadow_dda_steps = h[6];
    c->stats.loop_iterations = h[8];
    c->stats.active_lane_iterations = h[9];
    if (h[7]) {
        HIP_TRY(hipMemset(c->d_stats.get() + 7, 0, sizeof(unsigned long long)));
        return fail(AVR_ERR_STATE, "k_paths launched without its pass's camera stage (work heads not reset): pass not rendered");
    }
    return AVR_OK;
}

}  // extern "C"

#include "avr_render.hip"

extern "C" {

int avr_transmittance_device(avr_context *c, long long n, const float *p0, const float *p1, const float *lambda,
                             float *tr) {
    if (!c || n < 0 || (n > 0 && (!p0 || !p1 || !lambda || !tr))) return fail(AVR_ERR_ARG, "bad transmittance query");
    if (!c->has_medium) return fail(AVR_ERR_STATE, "medium required");
    if (n == 0) return AVR_OK;
    HIP_TRY(hipSetDevice(c->device));
    avr::Params p{};
    p.med = c->med;
    p.stats = c->d_stats.get();
    const int blocks = (int)std::min<long long>((n + 255) / 256, 8192);
    EV_MARK(t0);
    hipLaunchKernelGGL(avr::k_transmittance, dim3(blocks), dim3(256), 0, c->stream, p, n, p0, p1, lambda, tr);
    HIP_TRY(hipGetLastError());
    EV_MARK(t1);
    c->timed.push_back({t0, t1, &avr_stats::ms_shadow, false});
    return AVR_OK;
}

int avr_transmittance(avr_context *c, long long n, const float *p0, const float *p1, const float *lambda, float *tr) {
    if (!c || n < 0 || (n > 0 && (!p0 || !p1 || !lambda || !tr))) return fail(AVR_ERR_ARG, "bad transmittance query");
    if (n == 0) return AVR_OK;
    HIP_TRY(hipSetDevice(c->device));
    Arena<> scratch(c->stream);
    const auto r0 = scratch.reserve<float>(3 * (size_t)n), r1 = scratch.reserve<float>(3 * (size_t)n);
    const auto rl = scratch.reserve<float>(4 * (size_t)n), rtr = scratch.reserve<float>(4 * (size_t)n);
    HIP_TRY(scratch.commit());
    float *dp0 = scratch.get(r0), *dp1 = scratch.get(r1), *dl = scratch.get(rl), *dtr = scratch.get(rtr);
    HIP_TRY(hipMemcpyAsync(dp0, p0, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dp1, p1, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dl, lambda, 4 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const int rc = avr_transmittance_device(c, n, dp0, dp1, dl, dtr);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(tr, dtr, 4 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_sync(avr_context *c) {
    if (!c) return fail(AVR_ERR_ARG, "null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->tstream) HIP_TRY(hipStreamSynchronize(c->tstream));
    return AVR_OK;
}

int avr_get_stats(avr_context *c, avr_stats *out) {
    if (!c || !out) return fail(AVR_ERR_ARG, "null arg");
    HIP_TRY(hipSetDevice(c->device));
    int rc = fold_stats(c);
    if (rc) return rc;
    *out = c->stats;
    return AVR_OK;
}

int avr_reset_stats(avr_context *c) {
    if (!c) return fail(AVR_ERR_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    int rc = fold_stats(c);
    if (rc) return rc;
    c->stats = {};
    HIP_TRY(hipMemsetAsync(c->d_stats.get(), 0, sizeof(unsigned long long) * avr::kNumStats, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

static constexpr int kMetricBlocks = 1024;

static int film_image(avr_context *c, const avr::Mat3 &M, int fp16, float *d_out) {
    const long long np = (long long)c->film.bw * c->film.bh;
    hipLaunchKernelGGL(avr::k_film_image, dim3(blocks_for(np, 256, 4096)), dim3(256), 0, c->stream, c->film, M,
                       fp16, d_out);
    HIP_TRY(hipGetLastError());
    return AVR_OK;
}

int avr_film_image_device(avr_context *c, const float out_from_sensor[9], int fp16, float *d_out) {
    if (!c || !c->has_film || !out_from_sensor || !d_out) return fail(AVR_ERR_STATE, "no film or null argument");
    HIP_TRY(hipSetDevice(c->device));
    avr::Mat3 M;
    for (int i = 0; i < 9; ++i) M.m[i] = out_from_sensor[i];
    return film_image(c, M, fp16 ? 1 : 0, d_out);
}

int avr_film_set_reference(avr_context *c, const float *reference_rgb, const float out_from_sensor[9], int fp16) {
    if (!c || !c->has_film || !reference_rgb || !out_from_sensor) return fail(AVR_ERR_STATE, "no film or null argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t np = (size_t)c->film.bw * c->film.bh;
    c->d_reference.reset();
    c->d_image.reset();
    HIP_TRY(c->d_reference.alloc(3 * np));
    HIP_TRY(c->d_image.alloc(3 * np));
    if (!c->d_metric) HIP_TRY(c->d_metric.alloc((size_t)(kMetricBlocks + 1) * avr::kMetricSlots));
    HIP_TRY(hipMemcpyAsync(c->d_reference.get(), reference_rgb, 3 * np * sizeof(float), hipMemcpyHostToDevice, c->stream));
    for (int i = 0; i < 9; ++i) c->ref_out_from_sensor.m[i] = out_from_sensor[i];
    c->ref_fp16 = fp16 ? 1 : 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_film_metric(avr_context *c, int metric, float *out) {
    if (!c || !c->has_film || !out) return fail(AVR_ERR_STATE, "no film");
    if (!c->d_reference) return fail(AVR_ERR_STATE, "no reference image (avr_film_set_reference)");
    if (metric < 0 || metric > 3) return fail(AVR_ERR_ARG, "metric must be 0 MSE, 1 MAE, 2 MRSE, 3 ME");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = film_image(c, c->ref_out_from_sensor, c->ref_fp16, c->d_image.get()))) return rc;
    const int np = c->film.bw * c->film.bh;
    double *tot = c->d_metric.get() + (size_t)kMetricBlocks * avr::kMetricSlots;
    hipLaunchKernelGGL(avr::k_metric, dim3(kMetricBlocks), dim3(256), 0, c->stream, c->d_image.get(),
                       c->d_reference.get(), np, metric, c->d_metric.get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(avr::k_metric_final, dim3(1), dim3(64), 0, c->stream, c->d_metric.get(), kMetricBlocks, tot);
    HIP_TRY(hipGetLastError());
    double h[avr::kMetricSlots];
    HIP_TRY(hipMemcpyAsync(h, tot, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // / (Float(xres) * Float(yres)); ME rounds its sums to float first (image.cpp:573-577)
    const float npix = (float)c->film.bw * (float)c->film.bh;
    const int n = metric == 3 ? 9 : 3;
    for (int k = 0; k < n; ++k) out[k] = metric == 3 ? (float)h[k] / npix : (float)(h[k] / npix);
    return AVR_OK;
}

// FLIP for `imgtool diff --metric FLIP` (src/ext/flip/flip.cpp:1085-1112, ComputeFLIPError)
int avr_flip(avr_context *c, const float *test, const float *ref, int width, int height, float ppd, float *error) {
    if (!c || !test || !ref || !error || width < 1 || height < 1) return fail(AVR_ERR_ARG, "avr_flip: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    if (!(ppd > 0)) ppd = avr::flip::ppd_default();
    std::vector<float> sf, ef, pf;
    const int rs = avr::flip::spatial_filter(ppd, sf);
    const int rd = avr::flip::detection_filter(ppd, false, ef);
    (void)avr::flip::detection_filter(ppd, true, pf);
    const float cmax = avr::flip::max_distance();
    const size_t n = (size_t)width * height;
    const size_t nf = sf.size() + ef.size() + pf.size();
    std::vector<float> filt(nf);
    std::copy(sf.begin(), sf.end(), filt.begin());
    std::copy(ef.begin(), ef.end(), filt.begin() + sf.size());
    std::copy(pf.begin(), pf.end(), filt.begin() + sf.size() + ef.size());
    Arena<> scratch(c->stream);
    const auto rIn = scratch.reserve<float>(6 * n), rF = scratch.reserve<float>(nf), rOut = scratch.reserve<float>(n);
    const auto rYc = scratch.reserve<avr::flip::F4>(2 * n);
    HIP_TRY(scratch.commit());
    float *d_in = scratch.get(rIn), *d_f = scratch.get(rF), *d_out = scratch.get(rOut);
    avr::flip::F4 *d_yc = scratch.get(rYc);
    HIP_TRY(hipMemcpyAsync(d_in, test, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_in + 3 * n, ref, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_f, filt.data(), nf * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(avr::k_flip_prep, dim3(blocks_for((long long)n)), dim3(256), 0, c->stream, d_in, d_in + 3 * n,
                       (int)n, d_yc, d_yc + n);
    hipLaunchKernelGGL(avr::k_flip_error, dim3(blocks_for((long long)n)), dim3(256), 0, c->stream, d_yc, d_yc + n, width,
                       height, d_f, rs, d_f + sf.size(), d_f + sf.size() + ef.size(), rd, cmax, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(error, d_out, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_film_read(avr_context *c, double *rgb, double *w) {
    if (!c || !c->has_film || !rgb || !w) return fail(AVR_ERR_STATE, "no film");
    const size_t np = (size_t)c->film.bw * c->film.bh;
    HIP_TRY(hipMemcpyAsync(rgb, c->film.rgb_sum, 3 * np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(w, c->film.w_sum, np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_film_read_spectral(avr_context *c, double *bucket_sums, double *weight_sums) {
    if (!c || !c->has_film || c->film.nbuckets <= 0) return fail(AVR_ERR_STATE, "no spectral film");
    if (!bucket_sums || !weight_sums) return fail(AVR_ERR_ARG, "null buffer");
    const size_t nb = (size_t)c->film.bw * c->film.bh * c->film.nbuckets;
    HIP_TRY(hipMemcpyAsync(bucket_sums, c->film.bucket_sum, nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(weight_sums, c->film.bucket_w, nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_film_spectral_device_ptrs(avr_context *c, void **bucket_sums, void **weight_sums) {
    if (!c || !c->has_film || c->film.nbuckets <= 0 || !bucket_sums || !weight_sums)
        return fail(AVR_ERR_STATE, "no spectral film");
    *bucket_sums = c->film.bucket_sum;
    *weight_sums = c->film.bucket_w;
    return AVR_OK;
}

int avr_film_device_ptrs(avr_context *c, void **rgb, void **w) {
    if (!c || !c->has_film || !rgb || !w) return fail(AVR_ERR_STATE, "no film");
    *rgb = c->film.rgb_sum;
    *w = c->film.w_sum;
    return AVR_OK;
}

int avr_last_pass_samples(avr_context *c, float *L, float *lambda, float *pdf, long long n_max, int *first,
                          int *ns) {
    AVR_QUIESCE(c);
    if (!c || !c->has_film || !L || !lambda || !pdf || !first || !ns) return fail(AVR_ERR_ARG, "null arg");
    const long long n = (long long)c->film.bw * c->film.bh * c->last.S;
    if (n_max < n) return fail(AVR_ERR_ARG, "buffer too small for the last pass");
    if (n > 0 && c->last.persistent && c->last.order_gen != c->order_gen)
        return fail(AVR_ERR_STATE, "the pixel order changed since the last render (its records are in the old order)");
    if (n > 0 && c->last.persistent) {
        // k_paths' records (L), its camera stage's wavelengths and their pdfs as k_film evaluates them
        HIP_TRY(hipMemcpy(L, c->set.rec.get(), n * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(lambda, c->set.cam2.get(), n * sizeof(float4), hipMemcpyDeviceToHost));
        {
            avr::DevFilm f = c->film;
            hipLaunchKernelGGL(avr::k_lambda_pdfs, dim3(blocks_for(n)), dim3(256), 0, c->stream, f, c->set.cam2.get(), c->set.cam4.get(), n,
                               c->last.fast ? 1 : 0);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        HIP_TRY(hipMemcpy(pdf, c->set.cam4.get(), n * sizeof(float4), hipMemcpyDeviceToHost));
        if (!c->h_pix_slot.empty()) {   // slot order -> pixel order
            const long long np = (long long)c->film.bw * c->film.bh;
            std::vector<float> tmp(4 * (size_t)np);
            for (float *a : {L, lambda, pdf})
                for (long long sb = 0; sb < n; sb += np) {
                    std::memcpy(tmp.data(), a + 4 * sb, 4 * np * sizeof(float));
                    for (long long p = 0; p < np; ++p)
                        std::memcpy(a + 4 * (sb + p), tmp.data() + 4 * (size_t)c->h_pix_slot[(size_t)p], 4 * sizeof(float));
                }
        }
    } else if (n > 0) {
        HIP_TRY(hipMemcpy(L, c->ps.L, n * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(lambda, c->ps.lambda, n * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(pdf, c->ps.pdf, n * sizeof(float4), hipMemcpyDeviceToHost));
    }
    *first = c->last.base;
    *ns = c->last.S;
    return AVR_OK;
}

int avr_last_kernel(avr_context *c, char *buf, int cap) {
    if (!c || !buf || cap <= 0) return fail(AVR_ERR_ARG, "null arg");
    std::snprintf(buf, (size_t)cap, "%s", c->last.variant >= 0 ? c->kpaths_name[c->last.variant] : "");
    return AVR_OK;
}

int avr_last_pass_weights(avr_context *c, float *w, long long n_max) {
    AVR_QUIESCE(c);
    if (!c || !c->has_film || !w) return fail(AVR_ERR_ARG, "null arg");
    const long long n = (long long)c->film.bw * c->film.bh * c->last.S;
    if (n_max < n) return fail(AVR_ERR_ARG, "buffer too small for the last pass");
    if (n > 0 && c->last.persistent && c->filter_type != 0 && c->last.order_gen != c->order_gen)
        return fail(AVR_ERR_STATE, "the pixel order changed since the last render (its records are in the old order)");
    if (c->filter_type == 0) {
        for (long long i = 0; i < n; ++i) w[i] = 1.f;   // BoxFilter::Sample weight
    } else if (n > 0 && c->last.persistent) {
        std::vector<float> camw((size_t)n);
        HIP_TRY(hipMemcpy(camw.data(), c->set.camw.get(), n * sizeof(float), hipMemcpyDeviceToHost));
        const long long np = (long long)c->film.bw * c->film.bh;
        for (long long i = 0; i < n; ++i)
            w[i] = camw[c->h_pix_slot.empty() ? i : (i / np) * np + c->h_pix_slot[(size_t)(i % np)]];
    } else if (n > 0) {
        HIP_TRY(hipMemcpy(w, c->ps.weight, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return AVR_OK;
}

int avr_last_pass_rays(avr_context *c, float *o3, float *d3, float *u, long long n_max) {
    AVR_QUIESCE(c);
    if (!c || !c->has_film) return fail(AVR_ERR_ARG, "null arg");
    const long long n = (long long)c->film.bw * c->film.bh * c->last.S;
    if (n_max < n) return fail(AVR_ERR_ARG, "buffer too small for the last pass");
    if (n > 0 && !c->last.persistent)
        return fail(AVR_ERR_STATE, "the last pass was not a persistent one (the wavefront path consumes its rays)");
    if (n > 0 && c->last.order_gen != c->order_gen)
        return fail(AVR_ERR_STATE, "the pixel order changed since the last render (its records are in the old order)");
    if (n <= 0) return AVR_OK;
    // the camera stage's records: cam0 {o after interface_entry, u}, cam1 {d, .}
    std::vector<float> cam0(4 * (size_t)n), cam1(4 * (size_t)n);
    HIP_TRY(hipMemcpy(cam0.data(), c->set.cam0.get(), n * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cam1.data(), c->set.cam1.get(), n * sizeof(float4), hipMemcpyDeviceToHost));
    const long long np = (long long)c->film.bw * c->film.bh;
    for (long long i = 0; i < n; ++i) {
        const size_t src = (size_t)(c->h_pix_slot.empty() ? i : (i / np) * np + c->h_pix_slot[(size_t)(i % np)]);
        for (int k = 0; k < 3; ++k) {
            if (o3) o3[3 * i + k] = cam0[4 * src + k];
            if (d3) d3[3 * i + k] = cam1[4 * src + k];
        }
        if (u) u[i] = cam0[4 * src + 3];
    }
    return AVR_OK;
}

int avr_film_export_device(avr_context *c, void *dst) {
    if (!c || !c->has_film || !dst) return fail(AVR_ERR_STATE, "no film");
    const size_t np = (size_t)c->film.bw * c->film.bh;
    double *d = (double *)dst;
    HIP_TRY(hipMemcpyAsync(d, c->film.rgb_sum, 3 * np * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d + 3 * np, c->film.w_sum, np * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (c->film.nbuckets > 0)   // SpectralFilm: bucket sums then weights follow
        HIP_TRY(hipMemcpyAsync(d + 4 * np, c->film.bucket_sum, 2 * np * c->film.nbuckets * sizeof(double),
                               hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

// RGBFilm sums of several contexts (one per GPU, one process: pbrt's in-process multi-GPU
// render) SUM-reduced into the root context's film with RCCL over xGMI: rgb, weights and,
// for a SpectralFilm, the bucket sums — in place on the root.
int avr_film_reduce_rccl(avr_context **ctxs, int n, int root) {
    if (!ctxs || n < 1 || root < 0 || root >= n) return fail(AVR_ERR_ARG, "film reduce: bad context list");
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i] || !ctxs[i]->has_film) return fail(AVR_ERR_STATE, "film reduce: context without a film");
        const avr::DevFilm &a = ctxs[i]->film, &b = ctxs[root]->film;
        if (a.width != b.width || a.height != b.height || a.nbuckets != b.nbuckets || a.x0 != b.x0 || a.y0 != b.y0 ||
            a.bw != b.bw || a.bh != b.bh)
            return fail(AVR_ERR_ARG, "film reduce: films differ in resolution, pixel bounds or buckets");
        for (int j = 0; j < i; ++j)
            if (ctxs[j]->device == ctxs[i]->device) return fail(AVR_ERR_ARG, "film reduce: one context per GPU");
    }
    std::vector<int> devs(n);
    for (int i = 0; i < n; ++i) {
        devs[i] = ctxs[i]->device;
        HIP_TRY(hipSetDevice(devs[i]));
        HIP_TRY(hipStreamSynchronize(ctxs[i]->stream));
    }
    // communicators are created once per clique (ncclCommInitAll costs a bootstrap) and
    // cached on the contexts; a different context list releases the old cliques first
    const std::vector<avr_context *> clique(ctxs, ctxs + n);
    bool cached = true;
    for (int i = 0; i < n && cached; ++i) cached = ctxs[i]->comm && ctxs[i]->comm_group == clique;
    if (!cached) {
        for (int i = 0; i < n; ++i) release_comms(ctxs[i]);
        std::vector<ncclComm_t> fresh(n);
        if (ncclCommInitAll(fresh.data(), n, devs.data()) != ncclSuccess)
            return fail(AVR_ERR_HIP, "ncclCommInitAll failed");
        for (int i = 0; i < n; ++i) {
            ctxs[i]->comm = fresh[i];
            ctxs[i]->comm_group = clique;
        }
    }
    std::vector<ncclComm_t> comms(n);
    for (int i = 0; i < n; ++i) comms[i] = ctxs[i]->comm;
    const size_t np = (size_t)ctxs[root]->film.bw * ctxs[root]->film.bh;
    const size_t nb = (size_t)ctxs[root]->film.nbuckets;
    ncclResult_t r = ncclGroupStart();
    for (int i = 0; r == ncclSuccess && i < n; ++i) {
        avr::DevFilm &f = ctxs[i]->film;
        r = ncclReduce(f.rgb_sum, f.rgb_sum, 3 * np, ncclDouble, ncclSum, root, comms[i], ctxs[i]->stream);
        if (r == ncclSuccess) r = ncclReduce(f.w_sum, f.w_sum, np, ncclDouble, ncclSum, root, comms[i], ctxs[i]->stream);
        if (r == ncclSuccess && nb > 0)
            r = ncclReduce(f.bucket_sum, f.bucket_sum, 2 * np * nb, ncclDouble, ncclSum, root, comms[i], ctxs[i]->stream);
    }
    const ncclResult_t re = ncclGroupEnd();
    if (r == ncclSuccess) r = re;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n; ++i) {
        (void)hipSetDevice(devs[i]);
        const hipError_t ei = hipStreamSynchronize(ctxs[i]->stream);
        if (e == hipSuccess) e = ei;   // (every rank's stream is drained; the first error is kept)
    }
    if (r != ncclSuccess) return fail(AVR_ERR_HIP, std::string("film reduce: ") + ncclGetErrorString(r));
    if (e != hipSuccess) return fail(AVR_ERR_HIP, std::string("film reduce: ") + hipGetErrorString(e));
    return AVR_OK;
}

}  // extern "C"

#include "avr_graph_capi.hip"

// Not part of include/avr.h: the device memory this process holds through the library's buffers
// and scratch arenas, in bytes and in blocks (the tests' leak check)
extern "C" int avr_debug_live_device_bytes(unsigned long long *bytes, unsigned long long *blocks) {
    if (bytes) *bytes = avr::devmem::g_live_bytes.load();
    if (blocks) *blocks = avr::devmem::g_live_blocks.load();
    return AVR_OK;
}

#if defined(AVR_PROFILE_SECTIONS) || defined(AVR_PROBE_STATS)
// Variant builds only (not part of include/avr.h): read and clear the k_paths section cycles
// (or, with AVR_PROBE_STATS, the walk / gather probe counters)
// of this context (stats[kNumStats .. kNumStats + 4], written by every k_paths unit).
extern "C" int avr_debug_sections(avr_context *c, unsigned long long *out) {
    if (!c || !out) return fail(AVR_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->d_stats.get() + avr::kNumStats, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(c->d_stats.get() + avr::kNumStats, 0, 8 * sizeof(unsigned long long)));
    return AVR_OK;
}
#endif
