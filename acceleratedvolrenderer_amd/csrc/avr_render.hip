// avr_render.hip — the render path of the C-ABI: a render call's pass plan and kernel arguments
// (shared with the graph integrators, avr_graph_capi.hip), the persistent pass as a sequence of
// steps, the wavefront pass, and avr_render, which drives them. Included by avr_capi.hip (shares
// avr_context, fail(), HIP_TRY, fold_stats, walk_schedule). DESIGN §4 has the pass chain.

// The ZSobol pass table of sample indices [base, base + S): its entries hold the digits above
// the lowest plo bits, where the pass's indices differ
static int pass_plo(long long base, int S) {
    int plo = 0;
    while ((base >> plo) != ((base + S - 1) >> plo)) ++plo;
    return plo;
}
// The ZSobol tables' rows under the film's pixel bounds and the mask that maps a pixel's Morton
// code to its row (ZSobolParams::rowmask): Morton(W - 1, H - 1) + 1 rows and the code itself for
// the whole film, at most 4^ceil(log2 max(bw, bh)) rows for bounds inside it.
static uint32_t film_rowmask(const avr_context *c, size_t *rows) {
    const size_t full = (size_t)avr::smp::encode_morton2((uint32_t)c->film.width - 1, (uint32_t)c->film.height - 1) + 1;
    return avr::smp::zsobol_rowmask(c->film.bw, c->film.bh, full, rows);
}
// what a built table depends on (a table built ahead is used only when the pass's key equals it;
// avr_film_pixel_bounds drops the tables built ahead, so the bounds are not part of it)
static void ptab_key(const avr_context *c, const avr::smp::ZSobolParams &zs, long long base, int plo, long long *key) {
    const long long k[kPtabKey] = {base, plo, (long long)zs.log2spp, (long long)zs.seed,
                                   (long long)c->film.width * 65536 + c->film.height, c->zs_pdims,
                                   (long long)(uintptr_t)zs.upper, zs.dmax};
    for (int i = 0; i < kPtabKey; ++i) key[i] = k[i];
}
// Build the pass table (and the camera stage's compact copy) of [base, base + S) into buffer buf
// on stream s, with its level-A table when the two-level build applies. No room for a buffer:
// d_zs_ptab[buf] stays null (the pixel table / every digit per call serve the pass).
static int ptab_build(avr_context *c, hipStream_t s, const avr::smp::ZSobolParams &zs, long long base, int plo, int buf,
                      bool two_level) {
    const long long P = (long long)c->film.bw * c->film.bh;
    size_t prow;
    (void)film_rowmask(c, &prow);
    const size_t need_e = prow * (size_t)c->zs_pdims;
    // the same headroom policy as the fat / bricked density copies (alloc_if_room); a failed
    // query of the free memory counts as no room here
    if (need_e > c->d_zs_ptab[buf].size()) {
        if (c->d_zs_ptab[buf].alloc_if_room(need_e) != hipSuccess) (void)hipGetLastError();
        if (!c->d_zs_ptab[buf]) return AVR_OK;
    }
    // two-level build: the plo + 2 table is shared by the four passes whose indices agree above
    // plo + 2 bits; each pass then derives its own from it (not when the caller's passes stride
    // past each other's group: a sample shard's rank would rebuild it for every pass)
    const uint64_t *atab = nullptr;
    if (two_level && plo + 2 <= zs.log2spp) {
        if (need_e > c->d_zs_atab.size()) {
            for (long long &k : c->zs_akey) k = -1;
            // (no room: one-level build)
            if (c->d_zs_atab.alloc_if_room(need_e) != hipSuccess) (void)hipGetLastError();
        }
        if (c->d_zs_atab) {
            const long long key[6] = {base >> (plo + 2), plo, (long long)zs.log2spp, zs.seed,
                                      (long long)c->film.width * 65536 + c->film.height, c->zs_pdims};
            bool same = true;
            for (int k = 0; k < 6; ++k) same = same && key[k] == c->zs_akey[k];
            if (!same) {
                hipLaunchKernelGGL(avr::k_zsobol_pass_table,
                                   dim3(blocks_for(P * (c->zs_pdims / 2), 256, 256 * 64)), dim3(256), 0, s, zs,
                                   c->film.x0, c->film.y0, c->film.bw, c->film.bh, c->zs_pdims, plo + 2,
                                   (base >> (plo + 2)) << (plo + 2), c->d_zs_atab.get(), (const uint64_t *)nullptr,
                                   avr::fastdiv_make((uint32_t)(c->zs_pdims / 2)), avr::fastdiv_make((uint32_t)c->film.bw),
                                   (uint64_t *)nullptr);
                HIP_TRY(hipGetLastError());
                for (int k = 0; k < 6; ++k) c->zs_akey[k] = key[k];
            }
            atab = c->d_zs_atab.get();
        }
    }
    // the camera stage's six entries per pixel (dimensions 0, 1, 6..9) also as a compact
    // scanline-ordered copy (48 B per pixel), when the table holds them
    const size_t need_c = c->zs_pdims >= 10 ? 6 * (size_t)P : 0;
    // (no room: the camera reads the rows)
    if (c->d_zs_ctab[buf].reserve(need_c) != hipSuccess) (void)hipGetLastError();
    uint64_t *ctab = need_c ? c->d_zs_ctab[buf].get() : nullptr;
    hipLaunchKernelGGL(avr::k_zsobol_pass_table, dim3(blocks_for(P * (c->zs_pdims / 2), 256, 256 * 64)), dim3(256), 0, s,
                       zs, c->film.x0, c->film.y0, c->film.bw, c->film.bh, c->zs_pdims, plo, base, c->d_zs_ptab[buf].get(), atab,
                       avr::fastdiv_make((uint32_t)(c->zs_pdims / 2)), avr::fastdiv_make((uint32_t)c->film.bw), ctab);
    HIP_TRY(hipGetLastError());
    return AVR_OK;
}

// next free pool event (folds first when the pool is full)
static int next_event(avr_context *c, int *idx, hipStream_t s = nullptr) {
    if (c->ev_used >= 512) {
        int rc = fold_stats(c);
        if (rc) return rc;
    }
    if (c->ev_used == c->evpool.size()) {
        avr::devmem::Event e;
        HIP_TRY(hipEventCreate(&e.h));
        c->evpool.push_back(std::move(e));
    }
    *idx = (int)c->ev_used++;
    HIP_TRY(hipEventRecord(c->evpool[*idx], s ? s : c->stream));
    return AVR_OK;
}
#define EV_MARK(var)                      \
    int var;                              \
    do {                                  \
        int rc_ = next_event(c, &var);    \
        if (rc_) return rc_;              \
    } while (0)

// The pixel sampler of a render call (avr_render, avr_graph_render): the ZSobol range checks,
// the device selected, and the ZSobol pixel table rebuilt when the sampler or film changed.
static int render_sampler(avr_context *c, int spp_end, int seed, avr::smp::ZSobolParams *out) {
    avr::smp::ZSobolParams zs{};
    if (c->sampler_kind == 1) {
        // ZSobolSampler indexes (Morton(pixel) << log2(spp)) | sampleIndex: indices must stay
        // below the sampler's samplesPerPixel and the Sobol' index below 2^32
        if (spp_end > c->sampler_spp) return fail(AVR_ERR_ARG, "zsobol: sample index beyond samplesPerPixel");
        zs = avr::smp::zsobol_params(c->sampler_spp, c->film.width, c->film.height, seed);
        // SobolSample takes indices below 2^SobolMatrixSize = 2^52 (lowdiscrepancy.h:170)
        if (2 * zs.nBase4Digits - (zs.log2spp & 1) > 52)
            return fail(AVR_ERR_ARG, "zsobol: resolution x spp beyond the 2^52 Sobol' index range");
        // Morton(pixel) and the pixel-only digits (zsobol_upper, the pixel table) are 32-bit
        const int res = (int)avr::smp::round_up_pow2((uint32_t)std::max(c->film.width, c->film.height));
        if (2 * avr::smp::ilog2((uint32_t)res) > 32)
            return fail(AVR_ERR_ARG, "zsobol: film resolution beyond 65536 (Morton(pixel) exceeds 32 bits)");
    }
    HIP_TRY(hipSetDevice(c->device));
    if (c->sampler_kind == 1) {
        // the tables' rows: by the film's pixel bounds (the sampler's parameters above: by the film)
        size_t rows;
        zs.rowmask = film_rowmask(c, &rows);
        // The digits of GetSampleIndex above log2(spp) depend on (pixel, dimension) only:
        // tabulate them once per film/bounds/sampler (k_zsobol_table; avr_film_pixel_bounds resets the key), so each sampler call computes
        // the log2(spp)/2 sample digits plus one load instead of all nBase4Digits
        const int key[3] = {c->sampler_spp, c->film.width, c->film.height};
        if (c->zs_key[0] != key[0] || c->zs_key[1] != key[1] || c->zs_key[2] != key[2]) {
            // a table built ahead reads the pixel table: let it finish, and drop it
            if (c->tstream) HIP_TRY(hipStreamSynchronize(c->tstream));
            c->look.invalidate();
            c->d_zs_table.reset();
            for (int k = 0; k < 3; ++k) c->zs_key[k] = key[k];
            if (c->zs_dims > 0) {
                if (c->d_zs_table.alloc(rows * c->zs_dims) != hipSuccess) {
                    (void)hipGetLastError();   // no room: every call computes all digits
                } else {
                    EV_MARK(t0);
                    hipLaunchKernelGGL(avr::k_zsobol_table, dim3(blocks_for((long long)c->film.bw * c->film.bh *
                                                                            c->zs_dims, 256, 256 * 64)),
                                       dim3(256), 0, c->stream, zs, c->film.x0, c->film.y0, c->film.bw, c->film.bh,
                                       c->zs_dims, c->d_zs_table.get());
                    HIP_TRY(hipGetLastError());
                    EV_MARK(t1);
                    c->timed.push_back({t0, t1, &avr_stats::ms_setup, false});
                }
            }
        }
        zs.upper = c->d_zs_table.get();
        zs.dmax = c->d_zs_table ? c->zs_dims : 0;
    }
    // (padding bytes zeroed too, here and in pass_params: a pass takes camera records made ahead
    // only when its camera stage's arguments equal theirs byte for byte)
    std::memset(out, 0, sizeof *out);
    out->log2spp = zs.log2spp; out->nBase4Digits = zs.nBase4Digits; out->seed = zs.seed;
    out->rowmask = zs.rowmask;
    out->upper = zs.upper; out->dmax = zs.dmax;
    out->ptab = zs.ptab; out->pdims = zs.pdims; out->plo = zs.plo; out->ctab = zs.ctab;
    return AVR_OK;
}

// A render call's split into passes of S <= Smax sample indices over the P pixels of the film's bounds (P * S <=
// max_paths paths in flight), and the samples to allocate for its largest pass
struct PassPlan { long long P, Smax, need; };
static int pass_plan(const avr_context *c, bool persistent, int spp_begin, int spp_end, PassPlan *plan) {
    plan->P = (long long)c->film.bw * c->film.bh;
    if (plan->P > (1ll << 30)) return fail(AVR_ERR_ARG, "film too large");
    const long long maxp = c->max_paths_set ? c->max_paths : (persistent ? (64ll << 20) : c->max_paths);
    plan->Smax = std::max<long long>(1, maxp / plan->P);
    plan->need = plan->P * std::min<long long>(plan->Smax, std::max(1, spp_end - spp_begin));
    return AVR_OK;
}

// The kernel arguments of the pass [base, base + S), zeroed including padding before they are
// filled; zs from render_sampler. The records and camera stage are the primary camera set's.
static void pass_params(const avr_context *c, const avr::smp::ZSobolParams &zs, int seed, int max_depth, long long P,
                        long long base, int S, avr::Params *p) {
    std::memset(p, 0, sizeof *p);
    p->med = c->med;
    p->lights = c->lights;
    p->cam = c->cam;
    p->film = c->film;
    p->film.filter_type = c->filter_type;
    p->film.gauss = c->ftab;
    p->sampler_kind = c->sampler_kind;
    p->zs = zs;
    p->ps = c->ps;
    p->sh = c->sh;
    c->set.point(*p);
    p->max_depth = max_depth;
    p->seed = seed;
    p->pass_pixels = (int)P;
    p->div_pixels = avr::fastdiv_make((uint32_t)P);
    p->div_width = avr::fastdiv_make((uint32_t)c->film.bw);
    p->pass_samples = S;
    p->sample_base = (int)base;
    p->stats = c->d_stats.get();
}

// ZSobol quads in the camera stage: 4-aligned sample ranges, at most 8 lower base-4 digits
static int cam_quad(long long base, int S, const avr::smp::ZSobolParams &zs) {
    return (base % 4 == 0 && S % 4 == 0 && zs.log2spp <= 16) ? 1 : 0;
}
// k_paths' camera stage (k_paths_camera, one lane per sample) for the context's mode and sampler
// (the sampler variant is k_paths': avr_kpaths_slot.h)
using PassKernel = void (*)(avr::Params);
static PassKernel camera_stage_kernel(const avr_context *c, const avr::smp::ZSobolParams &zs) {
    static const PassKernel kcam[2][3] = {
        {avr::k_paths_camera<0, false>, avr::k_paths_camera<2, false>, avr::k_paths_camera<3, false>},
        {avr::k_paths_camera<0, true>, avr::k_paths_camera<2, true>, avr::k_paths_camera<3, true>}};
    // the general cameras (a thin lens, the spherical camera): their own instantiations, so that the
    // pinholes' hold none of it
    static const PassKernel kgen[2][3] = {
        {avr::k_paths_camera<0, false, 1>, avr::k_paths_camera<2, false, 1>, avr::k_paths_camera<3, false, 1>},
        {avr::k_paths_camera<0, true, 1>, avr::k_paths_camera<2, true, 1>, avr::k_paths_camera<3, true, 1>}};
    const int sv = avr::kp::sampler_index(avr::kp::sampler_arg(c->sampler_kind, avr::smp::zsobol_wide(zs)));
    return (avr::camera_general(c->cam) ? kgen : kcam)[c->render_mode ? 1 : 0][sv];
}

// k_film over the pass's pixels, timed into ms_film from event `from` (-1: from here). fast: the
// wavelength pdfs with the hardware exp (fast mode's wavelengths are the hardware log's)
static int launch_film(avr_context *c, const avr::Params &p, bool fast, int from = -1) {
    int rc = 0;
    if (from < 0 && (rc = next_event(c, &from))) return rc;
    static const PassKernel kfilm[2][2] = {{avr::k_film<false, false>, avr::k_film<true, false>},
                                           {avr::k_film<false, true>, avr::k_film<true, true>}};
    hipLaunchKernelGGL(kfilm[fast ? 1 : 0][c->film.nbuckets > 0 ? 1 : 0], dim3(blocks_for(p.pass_pixels)), dim3(256),
                       avr::film_lds_bytes(c->film.nbuckets), c->stream, p);
    HIP_TRY(hipGetLastError());
    EV_MARK(f1);
    c->timed.push_back({from, f1, &avr_stats::ms_film, false});
    return AVR_OK;
}

// k_camera (the wavefront kernels' and the graph integrators' camera rays), timed into
// ms_camera; *end: the event recorded behind it
static int launch_camera(avr_context *c, const avr::Params &p, int *end = nullptr) {
    const long long n0 = (long long)p.pass_pixels * p.pass_samples;
    EV_MARK(c0);
    static const PassKernel kcam[2][2] = {{avr::k_camera<false>, avr::k_camera<true>},
                                          {avr::k_camera<false, 1>, avr::k_camera<true, 1>}};
    hipLaunchKernelGGL(kcam[avr::camera_general(c->cam) ? 1 : 0][c->sampler_kind ? 1 : 0], dim3(blocks_for(n0)), dim3(256),
                       0, c->stream, p);
    HIP_TRY(hipGetLastError());
    EV_MARK(c1);
    c->timed.push_back({c0, c1, &avr_stats::ms_camera, false});
    if (end) *end = c1;
    return AVR_OK;
}

// What one avr_render call's passes share
struct RenderCall {
    int spp_begin, spp_end;
    avr::smp::ZSobolParams zs;   // render_sampler's (no pass table yet)
    PassPlan plan;
    // the stride between consecutive calls' first sample indices (S for pbrt's pass loop and the
    // one-GPU bench, N x S for a rank of an N-GPU sample shard): where the pass after this call's
    // last one is expected to start, for the pass table built ahead; 0 unknown
    long long call_stride;
    bool overlap_ok;             // a camera stage may run beside k_paths (avr_render)
};

// Persistent pass, step 1: the PCG32 advance table, Advance(s*65536) as an affine map state' =
// A*state + inc*H (rng.h:132-146: every step is linear in inc, so H = accPlus computed with
// inc = 1). Grown for both samplers, filled only for the one that reads it.
static int pass_advance_table(avr_context *c, long long base, int S) {
    // (two entries per sample; no drain of the stream in front of the free: hipFree waits for
    // queued work itself)
    HIP_TRY(c->d_advance.reserve(2 * (size_t)S));
    if (c->sampler_kind == 0) {   // read by the IndependentSampler's camera stage only
        hipLaunchKernelGGL(avr::k_advance, dim3((S + 255) / 256), dim3(256), 0, c->stream, c->d_advance.get(), (long long)base,
                           S);
        HIP_TRY(hipGetLastError());
    }
    return AVR_OK;
}

// Step 2: the ZSobol pass table: the digits of GetSampleIndex that the pass's sample indices
// [base, base + S) share (those above their lowest differing bits), for the first zs_pdims
// dimensions; the camera stage and k_paths then evaluate only the digits below (two MixBits at
// 64 indices per pass). The table the previous pass built ahead when it is this pass's (claim),
// else built here on the main stream. *have: p->zs names a table; *cam_ahead: the side stream
// made (or is making) camera records beside it.
static int pass_table(avr_context *c, const RenderCall &rc, long long base, int S, avr::Params *p, bool *have,
                      bool *cam_ahead) {
    *have = *cam_ahead = false;
    // rows (film_rowmask): Morton(w-1, h-1) + 1 of the whole film (up to ~4x the pixels of a
    // non-square one), fewer under pixel bounds: the table kernel indexes entries with 32 bits
    size_t rows;
    (void)film_rowmask(c, &rows);
    const long long prow = (long long)rows;
    if (!(c->sampler_kind == 1 && c->zs_pdims > 0 && rc.plan.P * c->zs_pdims < (1ll << 31) &&
          prow * c->zs_pdims < (1ll << 31)))
        return AVR_OK;
    const int plo = pass_plo(base, S);
    long long key[kPtabKey];
    ptab_key(c, rc.zs, base, plo, key);
    int buf = -1;
    HIP_TRY(c->look.claim(c->stream, c->ev_tab, key, c->cfg_gen, &buf, cam_ahead));
    *cam_ahead = *cam_ahead && rc.overlap_ok;
    if (buf < 0) {
        buf = 1 - c->tab_buf;
        int rc2 = ptab_build(c, c->stream, rc.zs, base, plo, buf, rc.call_stride == 0 || rc.call_stride == S);
        if (rc2) return rc2;
        if (!c->d_zs_ptab[buf]) return AVR_OK;
    }
    c->tab_buf = buf;
    p->zs.ptab = c->d_zs_ptab[buf].get();
    p->zs.ctab = c->zs_pdims >= 10 ? c->d_zs_ctab[buf].get() : nullptr;
    p->zs.pdims = c->zs_pdims;
    p->zs.plo = plo;
    *have = true;
    return AVR_OK;
}

// Step 3: the camera stage. It zeroes the work heads and stamps pass_gen into heads[8], and
// must come before k_paths on this stream: a k_paths launched without it renders nothing and
// makes the stats readback fail (stats[7]). Records made ahead (cam_ahead) are this pass's when
// the stage would be launched with the very arguments they were made with: then the camera sets
// swap and nothing is launched (they were made behind ev_tab, which this stream waited for).
// `from`: the event the stage's ms_camera interval starts at (before the pass table).
static int pass_camera_stage(avr_context *c, avr::Params *p, bool cam_ahead, int from, bool *taken) {
    *taken = false;
    if (cam_ahead) {
        avr::Params t = *p;
        c->alt.point(t);
        if (std::memcmp(&t, &c->look.params, sizeof t) == 0) {
            std::swap(c->set, c->alt);
            *p = t;
            *taken = true;
            return AVR_OK;
        }
    }
    // 16384 blocks (64 per CU, ~14 samples per thread at the bench's pass): the measured optimum
    // between one round of resident blocks and one sample per thread
    // (profiles/r06_ab_camera_grid.json)
    const int cgrid = blocks_for((long long)p->pass_pixels * p->pass_samples, 256, 256 * 64);
    hipLaunchKernelGGL(camera_stage_kernel(c, p->zs), dim3(cgrid), dim3(256), 0, c->stream, *p);
    HIP_TRY(hipGetLastError());
    EV_MARK(ec1);
    c->timed.push_back({from, ec1, &avr_stats::ms_camera, false});
    return AVR_OK;
}

// Step 4: k_paths, the instantiation for the context's mode, lights, medium and sampler, on its
// persistent grid; timed into ms_medium as the pass's one launch. With a camera stage beside it
// (cam_next) it is launched as four blocks per CU (the grid, and kOverlapLdsPad bytes of dynamic
// LDS nobody uses so that a fifth block does not fit a CU): the fifth wave slot of every SIMD
// and the LDS left take a camera block. *variant: the slot launched; *end: the event behind it.
static int pass_kpaths(avr_context *c, const avr::Params &p, bool cam_next, int *variant, int *end) {
    EV_MARK(e0);
    const int kv = avr::kp::select(c->render_mode != 0, c->n_image_lights > 0 || c->lights.mode != avr::kPickInfinite, c->med.type,
                                   c->sampler_kind, avr::smp::zsobol_wide(p.zs), c->med.emissive != 0, c->gray,
                                   c->med.fat != nullptr);
    const bool hold = cam_next && c->paths_grid[kv] > 4 * c->num_cus;
    hipLaunchKernelGGL(c->kpaths[kv], dim3(hold ? 4 * c->num_cus : c->paths_grid[kv]), dim3(256),
                       hold ? kOverlapLdsPad : 0, c->stream, p);
    HIP_TRY(hipGetLastError());
    EV_MARK(e1);
    c->timed.push_back({e0, e1, &avr_stats::ms_medium, true});
    *variant = kv;
    *end = e1;
    return AVR_OK;
}

// Step 6: the NEXT pass's table (sample indices [nb, nb + S): the next loop iteration's, or the
// next avr_render call's when the caller walks the indices in order) built ahead into the other
// buffer on the low-priority side stream: it waits for this pass's camera stage (ev_cam; the
// last reader of that buffer, k_paths of the previous pass, is then done too) and is dispatched
// as k_paths' blocks retire in its drain, instead of in front of the next camera stage. A pass
// whose key differs builds its own table (and this one is discarded). With cam_next, that pass's
// camera stage follows the table on the side stream, into the other camera set: its last
// readers, the previous pass's k_paths and k_film, came before ev_cam on the main stream. The
// pass is assumed to have this one's size and arguments (pcam: this pass's camera stage's); the
// pass itself checks that (look.params).
static int pass_build_ahead(avr_context *c, const RenderCall &rc, long long base, int S, const avr::Params &pcam,
                            bool cam_next) {
    const bool in_call = base + rc.plan.Smax < rc.spp_end || rc.call_stride == 0;
    const long long nb = in_call ? base + S : rc.spp_begin + rc.call_stride;
    const int nplo = pass_plo(nb, S);
    HIP_TRY(hipStreamWaitEvent(c->tstream, c->ev_cam, 0));
    const int tb = 1 - c->tab_buf;
    // (not timed: events around it would measure its wait for the drain too)
    int rc2 = ptab_build(c, c->tstream, rc.zs, nb, nplo, tb, in_call || rc.call_stride == S);
    if (rc2) return rc2;
    avr::Params q = pcam;
    const bool cam = cam_next && c->d_zs_ptab[tb];
    if (cam) {
        q.sample_base = (int)nb;
        q.pass_gen = (c->pass_gen + 1) & 0x7fffffff;
        q.cam_quad = cam_quad(nb, S, q.zs);
        q.zs = rc.zs;
        q.zs.ptab = c->d_zs_ptab[tb].get();
        q.zs.ctab = c->zs_pdims >= 10 ? c->d_zs_ctab[tb].get() : nullptr;
        q.zs.pdims = c->zs_pdims;
        q.zs.plo = nplo;
        c->alt.point(q);
        // timed on the side stream
        int sc0, sc1;
        if ((rc2 = next_event(c, &sc0, c->tstream))) return rc2;
        hipLaunchKernelGGL(camera_stage_kernel(c, pcam.zs), dim3(blocks_for((long long)q.pass_pixels * S, 256, 256 * 64)),
                           dim3(256), 0, c->tstream, q);
        HIP_TRY(hipGetLastError());
        if ((rc2 = next_event(c, &sc1, c->tstream))) return rc2;
        c->timed.push_back({sc0, sc1, &avr_stats::ms_camera, false});
    }
    // (recorded even when the buffer could not be allocated: nothing is published then, and no
    // pass waits for it)
    HIP_TRY(hipEventRecord(c->ev_tab, c->tstream));
    if (c->d_zs_ptab[tb]) {
        long long key[kPtabKey];
        ptab_key(c, rc.zs, nb, nplo, key);
        c->look.publish(key, tb, cam ? &q : nullptr, c->cfg_gen);
    }
    return AVR_OK;
}

// One pass of the persistent organisation: advance table, pass table (claimed or built), camera
// stage (taken or run), k_paths, k_film, then the next pass's table and camera stage built
// ahead. Everything on the context's stream except the last step (the side stream, between
// ev_cam and ev_tab).
static int render_pass_persistent(avr_context *c, const RenderCall &rc, long long base, int S, avr::Params &p) {
    int r = pass_advance_table(c, base, S);
    if (r) return r;
    p.advance = c->d_advance.get();
    walk_schedule(c, c->refill_min, c->dda_budget, &p.refill_min, &p.dda_budget, &p.refill_batch);   // defaults: measured optima
    p.pass_gen = ++c->pass_gen & 0x7fffffff;
    p.pix_order = c->d_pix_order.get();
    p.cam_quad = cam_quad(base, S, p.zs);
    EV_MARK(ec);
    bool have_table, cam_ahead, cam_taken;
    if ((r = pass_table(c, rc, base, S, &p, &have_table, &cam_ahead))) return r;
    if ((r = pass_camera_stage(c, &p, cam_ahead, ec, &cam_taken))) return r;
    const avr::Params pcam = p;   // the camera stage's arguments of this pass
    // build the next pass's ZSobol table ahead (ptab_spec), and its camera stage behind it
    const bool spec_next = have_table && c->ptab_spec != 0;
    if (spec_next) HIP_TRY(hipEventRecord(c->ev_cam, c->stream));
    const bool cam_next = spec_next && rc.overlap_ok && c->alt_cap >= rc.plan.P * S && c->alt_cap == c->rec_cap;
    int variant, e1;
    if ((r = pass_kpaths(c, p, cam_next, &variant, &e1))) return r;
    p.rec_mode = 1;   // k_film reads the records k_paths wrote (in slot order)
    p.pix_slot = c->d_pix_slot.get();
    p.fast = c->render_mode;
    if ((r = launch_film(c, p, c->render_mode != 0, e1))) return r;
    if (spec_next && (r = pass_build_ahead(c, rc, base, S, pcam, cam_next))) return r;
    LastPass lp;
    lp.persistent = true; lp.fast = c->render_mode == 1;
    lp.base = (int)base; lp.S = S; lp.order_gen = c->order_gen;
    lp.overlap = cam_taken; lp.variant = variant;
    c->last = lp;
    return AVR_OK;
}

// Ray binning (avr_set_ray_binning): counting-sort `count` queue entries (queue null: identity)
// by (majorant cell, octant) of their rays into d_bin_out; timed into ms_binning
static int bin_queue(avr_context *c, int nbins, long long count, const int *queue, const int *count_p, const float4 *o,
                     const float4 *d) {
    EV_MARK(s0);
    int *keys = c->d_bin_keys.get(), *hist = c->d_bin_hist.get();
    HIP_TRY(hipMemsetAsync(hist, 0, nbins * sizeof(int), c->stream));
    const int nbk = blocks_for(count);
    hipLaunchKernelGGL(avr::k_bin_count, dim3(nbk), dim3(256), 0, c->stream, c->med, queue, count_p, o, d, keys, hist);
    hipLaunchKernelGGL(avr::k_bin_scan, dim3(1), dim3(1024), 0, c->stream, hist, nbins);
    hipLaunchKernelGGL(avr::k_bin_scatter, dim3(nbk), dim3(256), 0, c->stream, queue, count_p, keys, hist,
                       c->d_bin_out.get());
    HIP_TRY(hipGetLastError());
    EV_MARK(s1);
    c->timed.push_back({s0, s1, &avr_stats::ms_binning, false});
    return AVR_OK;
}

// One pass of the wavefront organisation: k_camera, then depth iterations of {k_medium,
// k_shadow} over compacted queues until no path survives, then k_film. The host reads back the
// survivor count per depth to size the next launch and stop early.
static int render_pass_wavefront(avr_context *c, long long base, int S, avr::Params &p) {
    const long long n0 = (long long)p.pass_pixels * S;
    int r = launch_camera(c, p);
    if (r) return r;
    c->h_count[0] = (int)n0;
    int *const counts = c->d_counts.get();
    int *const queue[2] = {c->paths.queue[0].get(), c->paths.queue[1].get()};
    HIP_TRY(hipMemcpyAsync(counts, c->h_count, sizeof(int), hipMemcpyHostToDevice, c->stream));
    const int nbins = 8 * c->med.mres[0] * c->med.mres[1] * c->med.mres[2];
    const bool bin = c->ray_binning && nbins <= 8 * 4096;
    int cur = 0;
    long long count = n0;
    bool first = true;
    while (count > 0) {
        const int nxt = cur ^ 1;
        HIP_TRY(hipMemsetAsync(counts + nxt, 0, sizeof(int), c->stream));
        HIP_TRY(hipMemsetAsync(counts + 2, 0, sizeof(int), c->stream));
        p.queue_in = first ? nullptr : queue[cur];
        p.count_in = counts + cur;
        if (bin) {
            HIP_TRY(c->d_bin_keys.reserve((size_t)n0));
            HIP_TRY(c->d_bin_out.reserve((size_t)n0));
            if (!c->d_bin_hist) HIP_TRY(c->d_bin_hist.alloc((size_t)8 * 4096));
        }
        // camera rays keep their pixel order (already coherent); later depths are binned
        if (bin && !first) {
            if ((r = bin_queue(c, nbins, count, queue[cur], counts + cur, c->ps.o, c->ps.d))) return r;
            HIP_TRY(hipMemcpyAsync(queue[cur], c->d_bin_out.get(), (size_t)count * sizeof(int), hipMemcpyDeviceToDevice,
                                   c->stream));
        }
        p.queue_out = queue[nxt];
        p.count_out = counts + nxt;
        p.shadow_count = counts + 2;
        const int nb = blocks_for(count);
        EV_MARK(m0);
        if (c->sampler_kind) hipLaunchKernelGGL(avr::k_medium<true>, dim3(nb), dim3(256), 0, c->stream, p);
        else hipLaunchKernelGGL(avr::k_medium<false>, dim3(nb), dim3(256), 0, c->stream, p);
        HIP_TRY(hipGetLastError());
        EV_MARK(m1);
        c->timed.push_back({m0, m1, &avr_stats::ms_medium, true});
        p.sh_perm = nullptr;
        if (bin) {
            // the shadow rays k_medium just pushed, binned the same way (read through sh_perm)
            if ((r = bin_queue(c, nbins, count, nullptr, counts + 2, c->sh.o, c->sh.d))) return r;
            p.sh_perm = c->d_bin_out.get();
        }
        EV_MARK(m15);
        hipLaunchKernelGGL(avr::k_shadow, dim3(nb), dim3(256), 0, c->stream, p);
        HIP_TRY(hipGetLastError());
        EV_MARK(m2);
        c->timed.push_back({m15, m2, &avr_stats::ms_shadow, false});
        // the queue length decides the next launch: the wavefront organisation syncs here
        HIP_TRY(hipMemcpyAsync(c->h_count, counts + nxt, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        count = c->h_count[0];
        cur = nxt;
        first = false;
    }
    if ((r = launch_film(c, p, false))) return r;
    c->last = c->last.without_kpaths((int)base, S);
    return AVR_OK;
}

extern "C" int avr_render(avr_context *c, int spp_begin, int spp_end, int seed, int max_depth) {
    if (!c) return fail(AVR_ERR_ARG, "null context");
    if (!c->has_medium || !c->has_camera || !c->has_film) return fail(AVR_ERR_STATE, "medium, camera and film required");
    if (spp_begin < 0 || spp_end < spp_begin || max_depth < 0) return fail(AVR_ERR_ARG, "bad sample range");
    // every type-2 light needs its own image: a count of avr_light_image calls would let a map
    // replaced twice stand in for one never given, whose img and dist are null
    if (!image_lights_complete(c)) return fail(AVR_ERR_STATE, "image light without avr_light_image");
    if (!local_lights_complete(c)) return fail(AVR_ERR_STATE, "point or spot light without avr_light_local");
    if (c->light_sampler == 1 && c->lights.n > 0 && c->lights.mode != avr::kPickPower)
        return fail(AVR_ERR_STATE, "power light sampler: light weights incomplete");
    RenderCall rc;
    rc.spp_begin = spp_begin; rc.spp_end = spp_end;
    int r = render_sampler(c, spp_end, seed, &rc.zs);
    if (r) return r;
    // k_paths runs every medium type with every light type: GridMedium, RGBGridMedium and
    // the single-segment Homogeneous/CloudMedium keep the majorant in LDS (at most 4096
    // cells = pbrt's 16^3; larger grids take the wavefront kernels), NanoVDBMedium reads
    // its 64^3 majorant through L2
    const int mcells = c->med.mres[0] * c->med.mres[1] * c->med.mres[2];
    const bool persistent = c->kernel_mode == 0 &&
                            (((c->med.type != 3) && mcells <= 4096) || c->med.type == 3) &&
                            c->med.mres[0] <= 255 && c->med.mres[1] <= 255 && c->med.mres[2] <= 255;
    if ((r = pass_plan(c, persistent, spp_begin, spp_end, &rc.plan))) return r;
    if ((r = persistent ? ensure_records(c, rc.plan.need) : ensure_paths(c, rc.plan.need))) return r;
    // Pass overlap: only the parked k_paths instantiations (gray non-emissive GridMedium in the fat
    // layout without image lights) leave a block of the camera stage room beside four of their own on a CU;
    // only on the context's own stream (the side stream is ordered against it by events), and
    // only behind the ZSobol pass table built ahead
    rc.overlap_ok = persistent && c->pass_overlap && c->ptab_spec && c->sampler_kind == 1 &&
                    c->stream == c->own_stream && c->gray && c->med.type == 0 && !c->med.emissive && c->med.fat != nullptr &&
                    c->n_image_lights == 0 && c->lights.mode == avr::kPickInfinite;
    if (rc.overlap_ok) ensure_alt(c);
    EV_MARK(evStart);
    rc.call_stride = (c->prev_call_begin >= 0 && spp_begin > c->prev_call_begin) ? spp_begin - c->prev_call_begin : 0;
    c->prev_call_begin = spp_begin;
    for (long long base = spp_begin; base < spp_end; base += rc.plan.Smax) {
        const int S = (int)std::min<long long>(rc.plan.Smax, spp_end - base);
        avr::Params p;
        pass_params(c, rc.zs, seed, max_depth, rc.plan.P, base, S, &p);
        if ((r = persistent ? render_pass_persistent(c, rc, base, S, p) : render_pass_wavefront(c, base, S, p))) return r;
    }
    EV_MARK(evEnd);
    c->timed.push_back({evStart, evEnd, &avr_stats::ms_total, false});
    return AVR_OK;
}

