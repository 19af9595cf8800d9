/* avr.h — C-ABI of the MI355X-native volumetric path integrator (libavr_hip.so).
 *
 * Drop-in boundary for pbrt-v4's volumetric path in tsvdh/AcceleratedVolRenderer
 * (paths relative to /root/reference/src/pbrt). Plain C types only: opaque
 * handles, host pointers + sizes, int status codes (0 = ok), a thread-local
 * error string. No exceptions cross the ABI; buffers passed in are copied
 * during the call. One context per GPU; calls on one context are serialised
 * by the caller (pbrt drives Render() from one thread: cpu/render.cpp:159).
 *
 * Replaces:
 *   VolPathIntegrator::Render/Li/SampleLd   cpu/integrators.cpp:72-298, 962-1399
 *   SampleT_maj + DDAMajorantIterator        media.h:136-214, 730-806
 *   GridMedium SamplePoint/SampleRay/ctor    media.h:265-352, media.cpp:212-330
 *   WorkQueue push / ForAllQueued            wavefront/workqueue.h:41-172
 *   RGBFilm::AddSample / GetPixelRGB         film.h:232-316
 */
#ifndef AVR_H
#define AVR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVR_OK 0
#define AVR_ERR_ARG 1
#define AVR_ERR_HIP 2
#define AVR_ERR_STATE 3
#define AVR_ERR_INTERNAL 4 /* an invariant of the library failed: a bug, reported and never looped on */

#define AVR_TABLE_SIZE 471 /* DenselySampledSpectrum over 360..830 nm (spectrum.h:374-420) */

typedef struct avr_context avr_context;

/* Work counters and kernel times accumulated over every avr_render call since the context
 * was created or avr_reset_stats (pbrt's ReportKernelStats analogue,
 * wavefront/wavefront.cpp:47-56). Resolved when read: rendering never waits for them. */
typedef struct avr_stats {
    unsigned long long medium_lookups;  /* SamplePoint density fetches in k_medium   */
    unsigned long long medium_items_in; /* work items consumed by k_medium           */
    unsigned long long medium_items_out;/* survivors + shadow rays pushed by k_medium;
                                           k_paths: phase-function samples (real scatters
                                           that continue the path)                  */
    unsigned long long shadow_lookups;  /* density fetches in k_shadow               */
    unsigned long long shadow_items;    /* shadow rays traced                        */
    unsigned long long medium_dda_steps;
    unsigned long long shadow_dda_steps;
    unsigned long long medium_launches;
    unsigned long long loop_iterations;        /* k_paths: wave tracking iterations       */
    unsigned long long active_lane_iterations; /* k_paths: sum of busy lanes per iteration */
    double ms_camera, ms_medium, ms_shadow, ms_film; /* summed hipEvent times      */
    double ms_total;                                  /* first launch .. film done  */
    double ms_setup;   /* one-off device tables built by avr_render (ZSobol pixel table) */
    double ms_binning; /* wavefront ray binning (avr_set_ray_binning): key, scan, scatter passes */
} avr_stats;

/* Last error message of the calling thread ("" if none). */
const char *avr_last_error(void);

/* Context on HIP device `device` (one process per GPU; no implicit peer access).
 * `max_paths` bounds the paths in flight per pass (0 = default: 64M for the persistent
 * kernel, whose per-sample HBM state is 116 B — the 16-B radiance record plus the camera
 * stage's 6 x 16 B + 4 B, about 7.4 GB at 64M — 16M for the wavefront
 * kernels; at most 2^31 - 1: path ids are 32-bit, AVR_ERR_ARG above). */
int avr_context_create(int device, long long max_paths, avr_context **out);
/* Also releases the RCCL communicators the context shares with the other contexts of its
 * last avr_film_reduce_rccl list (see there: not concurrently with work on those contexts). */
int avr_context_destroy(avr_context *ctx);
/* Kernel organisation: 0 = persistent-wave megakernel k_paths (default: path state in
 * VGPRs, ballot-based lane refill), 1 = wavefront kernels k_camera/k_medium/k_shadow with
 * compacted SoA queues between events (pbrt wavefront decomposition). Same estimator. */
int avr_set_kernel_mode(avr_context *ctx, int mode);
/* Lookup trace (measurement): while d_points is non-null, the wavefront kernels append the
 * unit-box point of every GridMedium density fetch (float4 {x, y, z, 0}, fetch order) to
 * d_points (device, capacity cap) and count them in *d_count (device u64, zeroed by the
 * caller; counts past cap are not stored). NULL stops tracing. */
int avr_record_lookups(avr_context *ctx, void *d_points, long long cap, void *d_count);
/* The density fetch alone (SampledGrid::Lookup, containers.h:804-835, through the same fat /
 * linear layout code as the path kernels) over n unit-box points (device float4), results
 * to d_out (device, n floats); synchronous; *ms = the kernel's HIP-event time. */
int avr_density_fetch(avr_context *ctx, const void *d_points, long long n, float *d_out, float *ms);
/* A NanoVDBMedium grid's lookup alone (test probe): grid 0 = density, 1 = temperature. d_points
 * holds n device float4 medium-space points (what the kernels hand to the grid after
 * medium_from_render); d_out[i] = Grid::worldToIndexF then SampleFromVoxels<Tree, 1, false>
 * (media.h:627-636) of point i, through the lookup the path kernels call, so the density grid's
 * fat copy is read when avr_grid_layout_active says it exists (the temperature grid has the
 * apron blocks only). Synchronous; *ms = the kernel's HIP-event time (ms may be NULL).
 * Domain: finite points whose index-space coordinates lie within +-2^24 of the tree's voxels;
 * farther or non-finite points are the caller's error (the float -> int conversion of the
 * index is then unspecified). AVR_ERR_STATE: the current medium is not a NanoVDBMedium, or
 * grid 1 without a temperature grid; AVR_ERR_ARG: another grid, n < 0, a null buffer with
 * n > 0. n = 0 launches nothing. */
int avr_vdb_fetch(avr_context *ctx, int grid, const void *d_points, long long n, float *d_out, float *ms);
/* RGBGridMedium::SamplePoint alone (test probe; no render path uses it): points holds n render-space
 * points (host, n * 3), lambda their wavelengths in nm (host, n * 4). sigma_a4 / sigma_s4 / Le4
 * (host, n * 4 each; any may be NULL) receive sigmaScale * the sigma_a / sigma_s lookups (1 where
 * the medium has no such grid) and LeScale * the Le lookup (0 for a medium that is not emissive)
 * of media.h:377-403, one device lane per probe through the sample_point both kernel organisations
 * call: medium_from_render, Bounds3::Offset, then SampledGrid<RGB*Spectrum>::Lookup with the
 * spectrum sampled per tap. Works the same for avr_medium_rgbgrid and avr_medium_rgbgrid_device
 * grids. Synchronous. Domain: finite points (any distance from the box: taps outside the grid
 * convert to 0) and finite wavelengths. AVR_ERR_STATE: the current medium is not an RGBGridMedium;
 * AVR_ERR_ARG: n < 0, or null points / lambda with n > 0. n = 0 launches nothing. */
int avr_rgbgrid_probe(avr_context *ctx, long long n, const float *points, const float *lambda, float *sigma_a4,
                      float *sigma_s4, float *Le4);
/* Render mode for later renders (SURVEY.md §7 "replay / fast"): 0 = replay (default) — the
 * device evaluates log/atanh/cosh/sin/cos by the canonical f64 sequences and FastExp by pbrt's
 * CPU polynomial (util/math.h:450-471), so every sample replays the CPU VolPathIntegrator's bit
 * for bit; 1 = fast — the hardware v_log/v_exp/v_sin/v_cos (about 1 ulp) and a single
 * free-flight decision per candidate: the same estimator with different last bits, so parity
 * is statistical (film error within the Monte Carlo noise). Applies to the persistent kernel
 * (kernel mode 0); the wavefront kernels always replay. */
int avr_set_render_mode(avr_context *ctx, int mode);
/* Wavefront organisation (kernel mode 1) only: 1 = counting-sort the medium queue (depths
 * after the camera rays) and the shadow queue by (majorant cell of the ray origin, direction
 * octant) before each k_medium / k_shadow launch, so a wave's lanes gather from nearby voxels
 * (north star "density fetches coalesced along sorted ray packets"). Results unchanged. */
int avr_set_ray_binning(avr_context *ctx, int on);
/* NanoVDBMedium in the persistent kernel: 1 = stage a coarse occupancy level of the majorant
 * grid (one bit per cell pair, up to 64^3 cells) in LDS, so majorant-0 cells skip the L2 read
 * of the majorant; 0 (default) = read every cell's majorant (measured 2 % faster: occupied
 * cells then wait for the LDS bit before their L2 read). Rebuilds the current majorant.
 * Results unchanged (no reference counterpart: a DDAMajorantIterator, media.h:141-214, memory
 * schedule only). */
int avr_set_majorant_occupancy(avr_context *ctx, int on);
/* ZSobolSampler passes of the persistent kernel: 1 (default) = after launching a pass, build the
 * NEXT pass's ZSobol pass table (sample indices [base + S, base + 2S)) into a second buffer on a
 * low-priority side stream, where the dispatcher serves it as the pass's k_paths blocks retire;
 * the next pass (in the same avr_render call, or the next call when the caller's calls advance
 * by a fixed stride: pbrt's pass loop, a rank of a sample shard) then skips its own build. A
 * pass whose indices differ builds its table as before. 0 = build every table in front of its camera stage.
 * Results unchanged (a schedule of ZSobolSampler::GetSampleIndex's digits, samplers.h:225-330). */
int avr_set_pass_table_ahead(avr_context *ctx, int on);
/* Pass overlap (default 1): behind the table built ahead, the side stream also runs the next
 * pass's camera stage, into a second set of camera buffers, records and work heads (+116 B
 * per sample of the largest pass; without room for it the chain stays serial), while this
 * pass's k_paths runs held to four blocks per CU. Active for the k_paths instantiations with
 * a free wave slot (gray, non-emissive GridMedium without image lights or the power light
 * sampler), the ZSobol sampler with its pass table ahead, and the context's own stream. The
 * next pass is predicted like its table; it takes the records only if its camera stage would
 * be launched with byte-identical arguments and no setup call or readback came between, and
 * runs its own camera stage otherwise. Results do not depend on the setting.
 * avr_pass_overlap_active: whether the last pass took records made ahead. */
int avr_set_pass_overlap(avr_context *ctx, int on);
int avr_pass_overlap_active(avr_context *ctx);
/* k_paths' wave schedule has two parameters. A wave tracks its busy lanes until a service round
 * can serve at least `refill_min` lanes (or none is busy); the round runs each event handler
 * once for every lane that raised the event, and refills the lanes that wait for a new sample
 * once at least `refill_batch` of them wait (or none is busy). Waiting lanes count towards the
 * service threshold only when the round will refill them. Neither changes results.
 * avr_set_refill_min: the service threshold, 1..64 lanes; larger values batch the per-event
 * handlers across more lanes and leave more lanes idle meanwhile.
 * 0 = default (the measured optima in both render modes: 32; 20 for a non-emissive
 * NanoVDB medium at pbrt's 64^3 majorant, whose longer DDA walks favour smaller batches;
 * 16 for an RGBGridMedium; 48 for a GridMedium majorant of at most 2 cells per axis, e.g.
 * fast mode's tuned 1^3, whose one-cell walks leave the handlers dominant). */
int avr_set_refill_min(avr_context *ctx, int lanes);
/* avr_set_refill_batch: the fewest waiting lanes for which a service round refills, 1..64
 * (1: every round refills whatever waits; a value above the service threshold refills only
 * when no lane is busy). 0 = default: 1 for a gray, non-emissive GridMedium (measured: idle
 * lanes cost more than the refill's four loads); every other kind (emissive or chromatic grids,
 * NanoVDB, RGB grids, homogeneous media) keeps the coupled schedule, which refills at the
 * service threshold and counts every waiting lane towards it. The coupled schedule is a
 * default only: no value selects it, and `lanes` equal to the service threshold is not it (the
 * waiting lanes then do not count towards the threshold). To compare against it on a kind
 * whose default is 1, build the library with -DAVR_COUPLED_DEFAULT (python -m
 * acceleratedvolrenderer_amd.build <variant> -DAVR_COUPLED_DEFAULT). AVR_ERR_ARG outside 0..64. */
int avr_set_refill_batch(avr_context *ctx, int lanes);
/* k_paths: majorant-grid cells a lane may cross per tracking iteration before yielding to
 * the wave (0 = default: 10 for majorant grids up to 16^3, 32 for finer ones and for
 * RGBGridMedium, 28 for a non-emissive NanoVDB medium at 64^3 — measured optima); bounds the
 * divergence of the DDA walk. No effect on results. */
int avr_set_dda_budget(avr_context *ctx, int cells);
/* Density layout for the NEXT avr_medium_grid* / avr_medium_nanovdb call: 1 (default) also
 * builds a "fat" footprint copy — GridMedium: entry (ix,iy,iz) holds the 8 trilinear taps as
 * 32 contiguous bytes, (n+1)^3 x 32 B; NanoVDBMedium: the same 32 B per base voxel of every
 * 9^3 apron block of the density grid (512 x 32 B per block) — built on device if it fits in
 * free HBM with 8 GiB to spare, so a density fetch is one 32-B access in one cache line; 0
 * keeps only pbrt's linear layout (containers.h:834) / the apron blocks; 2 (GridMedium) builds a
 * bricked copy instead — 8^3 base voxels per brick with a +1 apron (9^3 floats, padded to 736),
 * bricks x-fastest, so a footprint's 8 taps lie in one brick (4 x 8 B within 368 B), 1.42x the
 * grid. Results are bit-identical in every layout. */
int avr_set_grid_layout(avr_context *ctx, int layout);
/* The current medium's density copy: 1 fat, 2 bricked, 0 none (pbrt's linear layout only). */
int avr_grid_layout_active(avr_context *ctx);
/* The persistent kernel's pixel order (SURVEY §7 step 6 / north star "density-grid fetches
 * coalesced along sorted ray packets"): `order` lists every pixel of the current film once
 * (row-major ids); within each sample index of a pass the camera stage and k_paths hand
 * pixels to lanes in that order, so consecutive lanes start coherent camera rays (e.g.
 * sorted by the majorant cell where the ray enters the medium). NULL restores scanline
 * order; a new film resets it. Results are identical in any order (per-pixel sums still
 * add the pixel's samples in sampleIndex order). */
int avr_set_pixel_order(avr_context *ctx, const int *order, long long n);
/* Run all work of this context on `hip_stream` (a hipStream_t; NULL = the context's own stream).
 * Drains the previous stream and the side stream first and drops what was built ahead; on a
 * caller's stream every pass runs its stages in series (no pass overlap). */
int avr_set_stream(avr_context *ctx, void *hip_stream);

/* GridMedium (media.h:271-275, media.cpp:249-330). density is nx*ny*nz floats,
 * x fastest ((z*ny + y)*nx + x, util/containers.h:830-835). sigma_a/sigma_s/Le are
 * DenselySampled tables already scaled (sigmaScale / LeNorm folded in, as the ctor's
 * Scale() calls do). Le may be NULL (non-emissive). Lescale is the LeScale grid
 * (lnx*lny*lnz, LeNorm folded in) and may be NULL when Le is NULL.
 * Transforms are row-major 4x4 (renderFromMedium and its inverse).
 * The majorant grid (majorant_res, pbrt uses 16^3, media.cpp:229) is built on device. */
int avr_medium_grid(avr_context *ctx, const float *density, int nx, int ny, int nz, const float bounds[6],
                    const float render_from_medium[16], const float medium_from_render[16],
                    const float *sigma_a, const float *sigma_s, float g, const float *Le, const float *Lescale,
                    int lnx, int lny, int lnz, const int majorant_res[3]);
/* Same, but the density already lives in device memory of this context's GPU
 * (e.g. a 4 GiB grid generated on device). The caller keeps ownership and must keep
 * it alive while the context renders. */
int avr_medium_grid_device(avr_context *ctx, const float *d_density, int nx, int ny, int nz, const float bounds[6],
                           const float render_from_medium[16], const float medium_from_render[16],
                           const float *sigma_a, const float *sigma_s, float g, const float *Le,
                           const float *Lescale, int lnx, int lny, int lnz, const int majorant_res[3]);
/* Attach a temperature grid (nx*ny*nz f32, same layout as the density) to the current
 * GridMedium: emission Le = LeScale(p) * BlackbodySpectrum(T)(lambda) with
 * T = (temperature(p) - offset) * scale where T > 100 K (media.h:299-316, media.cpp:
 * 256-329: "temperature", "temperaturescale", "temperatureoffset"). The medium must have
 * been created without an Le spectrum (pbrt rejects both). */
int avr_medium_temperature(avr_context *ctx, const float *temperature, float temperature_scale,
                           float temperature_offset);
/* HomogeneousMedium (media.h:217-262, Create media.cpp:165-210) filling the interface box
 * `bounds` (medium space): constant sigma_a/sigma_s tables (sigmaScale folded in), g, and
 * optionally Le (471, LeScale folded in; null = not emissive). Its majorant segment is the
 * box crossing with sigma_maj = sigma_t (HomogeneousMajorantIterator). */
int avr_medium_homogeneous(avr_context *ctx, const float bounds[6], const float render_from_medium[16],
                           const float medium_from_render[16], const float *sigma_a, const float *sigma_s, float g,
                           const float *Le);
/* CloudMedium (media.h:430-528, Create media.cpp:455-485): procedural density (Perlin noise;
 * parameters density, wispiness, frequency) inside `bounds`, one majorant segment per ray
 * with sigma_maj = sigma_t. */
int avr_medium_cloud(avr_context *ctx, const float bounds[6], const float render_from_medium[16],
                     const float medium_from_render[16], const float *sigma_a, const float *sigma_s, float g,
                     float density, float wispiness, float frequency);
/* One NanoVDB FloatGrid as NanoVDBMedium reads it (media.h:624-672; NanoVDB is the
 * un-vendored openvdb@414bed84 feature/nanovdb submodule): the 8^3 leaf nodes (origin =
 * index coordinate of the leaf's voxel (0,0,0), multiples of 8; 512 values each, x-major
 * ((x&7)*8 + (y&7))*8 + (z&7) as LeafNode stores them), the constant tiles of the upper tree
 * levels (origin and edge length in voxels, multiples of 8), the background value returned
 * everywhere else, the active-voxel index bbox (inclusive, GridData::mIndexBBox) and the map:
 * index->world as a row-major 3x4 (Map::mMatD with mVecD as the last column) and the inverse
 * 3x3 (Map::mInvMatD); the float copies worldToIndexF uses are their roundings, as Map::set
 * makes them. World bbox = the map of the corners of [min, max + 1], each row evaluated
 * ((m0*x + m1*y) + m2*z) + t in f64. */
typedef struct avr_vdb_grid {
    int n_leaves;
    const int *leaf_origin;      /* 3 per leaf */
    const float *leaf_values;    /* 512 per leaf */
    int n_tiles;
    const int *tile_origin;      /* 3 per tile (may be NULL when n_tiles == 0) */
    const int *tile_size;        /* 1 per tile */
    const float *tile_value;     /* 1 per tile */
    float background;
    int index_bbox[6];           /* min xyz, max xyz */
    double index_to_world[12];
    double world_to_index[9];
} avr_vdb_grid;
/* NanoVDBMedium (media.h:602-685, ctor media.cpp:511-616, Create media.cpp:618-665):
 * density grid, optional temperature grid (NULL = not emissive), sigma tables with
 * sigmaScale folded in, g, LeScale, temperatureoffset, temperaturescale. Bounds are the
 * density grid's world bbox (union the temperature grid's); the 64^3 majorant is built on
 * the device with pbrt's one-voxel filter slop. Replaces NanoVDBMedium::Create's
 * readGrid + ctor: the caller hands over the tree it read. */
int avr_medium_nanovdb(avr_context *ctx, const avr_vdb_grid *density, const avr_vdb_grid *temperature,
                       const float render_from_medium[16], const float medium_from_render[16],
                       const float *sigma_a, const float *sigma_s, float g, float Lescale,
                       float temperature_offset, float temperature_scale);
/* RGBGridMedium (media.h:355-427, ctor media.cpp:339-378, Create media.cpp:380-453): an
 * nx*ny*nz grid (x fastest) on the box `bounds` whose voxels hold RGBUnboundedSpectrum
 * sigma_a / sigma_s and RGBIlluminantSpectrum Le as 4 floats {c0, c1, c2, scale} — the
 * RGBSigmoidPolynomial coefficients RGBColorSpace::ToRGBCoeffs gave the caller and the
 * spectrum's scale (spectrum.cpp:236-247). sigma_a or sigma_s may be NULL (treated as 1);
 * Le (NULL = none) needs sigma_a and the colour space's illuminant table (471, e.g. D65
 * for sRGB). sigma_scale is "scale", Le_scale "Lescale". The 16^3 majorant
 * sigma_scale * (max sigma_a + max sigma_s) is built on the device. */
int avr_medium_rgbgrid(avr_context *ctx, int nx, int ny, int nz, const float bounds[6],
                       const float render_from_medium[16], const float medium_from_render[16],
                       const float *sigma_a, const float *sigma_s, float sigma_scale, float g, const float *Le,
                       const float *illuminant, float Le_scale);
/* Same, but sigma_a / sigma_s / Le are float4 arrays already in device memory of this context's
 * GPU (e.g. a 1024^3 grid generated on device, 16 GiB per field); the caller keeps ownership
 * and keeps them alive while the context renders. */
int avr_medium_rgbgrid_device(avr_context *ctx, int nx, int ny, int nz, const float bounds[6],
                              const float render_from_medium[16], const float medium_from_render[16],
                              const float *d_sigma_a, const float *d_sigma_s, float sigma_scale, float g,
                              const float *d_Le, const float *illuminant, float Le_scale);
/* Medium interface of the current medium (pbrt: a shape with no material
 * whose MediumInterface has this medium inside and none outside, interaction.cpp:91-97
 * SkipIntersection, shapes.h:152-200 Sphere). radius > 0: a sphere of that radius at `center`
 * (render space) bounds the medium — camera rays start their first segment where they enter
 * it, every segment and shadow ray ends at its exit, rays that miss it see no medium (the
 * medium's SampleT_maj still clips to its bounds box, media.h:325-328); radius <= 0 returns
 * to the default model (the bounds box is the interface). Reset by every avr_medium_* call.
 * Both kernel organisations. */
int avr_medium_boundary_sphere(avr_context *ctx, const float center[3], float radius);
/* A convex polyhedral medium interface (e.g. a convex triangle mesh — a box mesh, a prism —
 * given by its face planes): n_planes half-spaces {nx, ny, nz, h} in render space, the
 * medium inside every n.p <= h (outward normals, 1..256 planes; 0 returns to the box). Same
 * semantics as the sphere; crossings by the parametric slab clip (vecmath.h:1547-1571
 * generalised), not pbrt's watertight triangle test, so paths match pbrt statistically. */
int avr_medium_boundary_convex(avr_context *ctx, const float *planes, int n_planes);
/* The medium bounds the last avr_medium_* call set (medium space, min xyz then max xyz). */
int avr_medium_bounds(avr_context *ctx, float bounds[6]);
/* Fill d_out[first .. first+count) of an n^3 grid with CloudMedium::Density
 * (media.h:496-520) at voxel centres (i+0.5)/n — the synthetic S-cloud input. */
int avr_generate_cloud(avr_context *ctx, float *d_out, int n, long long first, long long count, float density,
                       float wispiness, float frequency);
/* Fill voxels [first, first + count) of three n^3 float4 device arrays with the synthetic
 * RGB-coefficient explosion (BASELINE config C5's stand-in as an RGBGridMedium): {c0, c1, c2,
 * scale} of sigma_a, sigma_s and Le at voxel centres (i + 0.5) / n; each pointer is the
 * array's element `first`. */
int avr_generate_rgb_explosion(avr_context *ctx, float *d_sigma_a, float *d_sigma_s, float *d_Le, int n,
                               long long first, long long count);
/* Copy the device majorant grid to host (mres product floats). */
int avr_read_majorant(avr_context *ctx, float *out);
/* Rebuild the current medium's majorant grid at res[3] cells (1..255 per axis) from the
 * medium's own data (GridMedium / RGBGridMedium / NanoVDBMedium; the single-segment media
 * refuse). pbrt fixes 16^3 for grids (media.cpp:229) and 64^3 for NanoVDB (media.cpp:521):
 * replay parity with pbrt assumes those; any conservative majorant gives the same estimator
 * in expectation (SURVEY §7 "fast": tuned majorant, statistical parity). The persistent
 * kernel keeps grids of up to 4096 cells in LDS; finer grid majorants run the wavefront kernels. */
int avr_set_majorant_res(avr_context *ctx, const int res[3]);
/* The "tuned majorant": render the probe sample range [spp_begin, spp_end) twice per
 * candidate resolution (n triples in `candidates`; candidates ascending, then descending),
 * timed with HIP events on the context stream, keep the fastest (chosen[3]; each candidate's
 * faster probe in ms[n] when non-null). The film sums are restored and the work counters
 * reset afterwards; no pass table is built ahead during the probes. */
int avr_tune_majorant(avr_context *ctx, const int *candidates, int n, int spp_begin, int spp_end, int seed,
                      int max_depth, int chosen[3], float *ms);
/* k_paths' lane schedule chosen on the device for the current scene (replaces fixed
 * per-medium defaults): render the probe sample range twice per (refill lanes, DDA cells)
 * candidate pair (the faster probe counts), refill[i] x dda[j] (0 = the library default for either), timed with HIP
 * events on the context stream, and keep the fastest (chosen[2] = {refill, dda}; the nr*nd
 * probe times in ms[i * nd + j] when non-null) — except that the default pair (0, 0), when
 * listed (else the current schedule, when listed), is kept unless the fastest probe beats
 * every probe of that same effective schedule (e.g. refill 0 and refill 32 where 32 is the
 * default) by more than 2 % (the probes' run-to-run spread), so repeated runs choose the same
 * schedule. Film sums restored and work counters reset
 * afterwards, as avr_tune_majorant. The schedule never changes results, only how a wave
 * batches its lanes' events and walks. */
int avr_tune_walk(avr_context *ctx, const int *refill, int nr, const int *dda, int nd, int spp_begin, int spp_end,
                  int seed, int max_depth, int chosen[2], float *ms);

/* Lights (lights.h:244-305 DistantLight, lights.cpp:950-972 UniformInfiniteLight).
 * type 0 = distant: w = render-space unit vector towards the light
 *          (Normalize(renderFromLight(0,0,1)), lights.h:287); type 1 = uniform infinite;
 * type 2 = image infinite (then avr_light_image); type 3 = point, type 4 = spot (lights.h:191-236,
 * 741-797; then avr_light_local; w is ignored and L is the intensity table I).
 * L = n tables of 471 floats; scale = final light scale (1/SpectrumToPhotometric folded in).
 * scene_radius = Bounds3::BoundingSphere radius of the scene bounds (lights.h:280). */
int avr_lights(avr_context *ctx, int n, const int *types, const float *w3, const float *L, const float *scale,
               float scene_radius);
/* ImageInfiniteLight (lights.h:552-640, ctor lights.cpp:1007-1040, Create lights.cpp:1527-1660)
 * for light `index` of the last avr_lights call, which lists it with type 2 (its L table is
 * ignored; `scale` is the final scale: "scale" / SpectrumToPhotometric(illuminant), times the
 * "illuminance" factor when given). A res x res equal-area octahedral map: per pixel the
 * RGBIlluminantSpectrum {c0, c1, c2, scale} of ClampZero(rgb) in the image's colour space,
 * `distribution` = Image::GetSamplingDistribution() (res*res, row y), the colour space's
 * illuminant (471) and renderFromLight / its inverse (row-major 4x4, the 3x3 part is used).
 * The library builds the compensated PiecewiseConstant2D that SampleLi / PDF_Li use with
 * allowIncompletePDF (VolPath always passes true). Scenes with image lights render with
 * the wavefront kernels. */
int avr_light_image(avr_context *ctx, int index, int res, const float *pixel_coeffs, const float *distribution,
                    const float *illuminant, const float render_from_light[16], const float light_from_render[16]);

/* PointLight / SpotLight for light `index` of the last avr_lights call, which lists it with type 3
 * or 4: renderFromLight and its inverse (row-major 4x4) and the spot light's
 * cos(Radians(falloffStart)), cos(Radians(totalWidth)). A point light passes cosines that make the
 * cone everything (1 and -1); they are not read. The lights are delta-position lights: NEE samples
 * them at the scatter point (Li = scale * I / r^2, times SmoothStep of the cone for the spot light),
 * they are invisible to camera rays and escape nothing. A render with a local light that lacks
 * this call returns AVR_ERR_STATE. Scenes with local lights run k_paths' general instantiations,
 * as scenes with image lights do. */
int avr_light_local(avr_context *ctx, int index, const float render_from_light[16], const float light_from_render[16],
                    float cos_falloff_start, float cos_falloff_end);

/* VolPath's light sampler (VolPathIntegrator::Create "lightsampler", integrators.cpp:1402-1420;
 * LightSampler::Create, lightsamplers.cpp:22-37): 0 = "bvh" (default) or "uniform" — identical
 * for infinite lights (lightsamplers.h:266-277, 35-50); 1 = "power": PowerLightSampler
 * (lightsamplers.h:63-99, lightsamplers.cpp:76-96), lights picked by an AliasTable over
 * Average(Phi(lambda) / pdf) at SampleVisible(0.5) (DistantLight / UniformInfiniteLight /
 * ImageInfiniteLight / PointLight / SpotLight::Phi, lights.cpp:216, 974, 1042, 164, 1365). Kept
 * across avr_lights calls; a power render needs every image light's avr_light_image first.
 * With a point or spot light in the list, 0 is pbrt's whole BVHLightSampler (lightsamplers.h:
 * 259-404): the infinite lights share pInfinite = nInf / (nInf + 1) and the rest goes to a
 * traversal of the light BVH by CompactLightBounds::Importance at the scatter point; the tree is
 * built on the host (lightsamplers.cpp:109-238) whenever the list or the sampler changes, without
 * the lights of zero power. 2 = "uniform": UniformLightSampler over the whole list
 * (lightsamplers.h:35-50); for lists of infinite lights 0 and 2 are the same pick. */
int avr_light_sampler(avr_context *ctx, int kind);

/* Readbacks of the light stage (replay checks; no render path uses them).
 * avr_light_probe runs, for light `index` of the last avr_lights call and n probes, the device
 * functions the path kernels call: SampleLi with allowIncompletePDF = true at (u0, u1) (u2, n*2)
 * gives the render-space wi (wi3, n*3), its pdf (pdf_sample, n) and Ls (Ls4, n*4) at the
 * wavelengths lambda4 (n*4); PDF_Li and Le of the escaping render-space direction w3 (n*3) give
 * pdf_li (n) and Le4 (n*4). A distant light samples its direction with pdf 1 and has PDF_Li and Le
 * 0; a uniform infinite light reports no sample (pdf_sample 0, wi and Ls 0), PDF_Li 0 and
 * Le = scale * L(lambda); an image light whose map pdf is 0 at (u0, u1) reports no sample. Any
 * output may be NULL. AVR_ERR_STATE while a type-2 light lacks its avr_light_image.
 * avr_light_probe and avr_light_pick change no result but are no free readbacks: like every call that
 * touches the light list they wait for the context's streams and drop camera records made ahead
 * for the next pass, which that pass then makes again.
 * avr_light_pick: the light sampler's pick for n draws u: idx (n; -1: no light) and its PMF (n).
 * avr_light_sampler_table (host only): per light the sampler's bin {q, p, alias}: the AliasTable
 * of the power sampler, or q = 1, p = 1 / n, alias = -1 for "bvh" / "uniform" (with a point or
 * spot light in the list the "bvh" PMF depends on the reference point: avr_light_pick_at). */
int avr_light_probe(avr_context *ctx, int index, int n, const float *u2, const float *w3, const float *lambda4,
                    float *wi3, float *pdf_sample, float *Ls4, float *pdf_li, float *Le4);
int avr_light_pick(avr_context *ctx, int n, const float *u, int *idx, float *pmf);
int avr_light_sampler_table(avr_context *ctx, float *q, float *p, int *alias);
/* The same with a reference point per probe (p3, n*3, render space), which local lights and the
 * light BVH depend on. avr_light_probe_at: SampleLi of light `index` at p: wi3 (n*3), pdf_sample
 * (n; 0: no sample, e.g. outside a spot light's cone), Ls4 (n*4) and the distance to the light
 * (dist, n; 2 x scene_radius for the infinite lights, the length of their shadow ray).
 * avr_light_pick_at: the light sampler's pick at p for the draw u.
 * avr_light_bvh (host only): the light BVH of sampler 0: *n_nodes nodes (at most 15) with, per
 * node, phi, the decoded direction w (w3), the two quantised cosines (qcos: o, e), the quantised
 * box (qb: min xyz, max xyz), the second child's node index or the leaf's light index (link) and
 * the leaf flag; all_bounds: allLightBounds (pMin, pMax); *n_infinite the number of infinite
 * lights. Any output may be NULL. No tree (no local light of non-zero power): *n_nodes = 0. */
int avr_light_probe_at(avr_context *ctx, int index, int n, const float *u2, const float *p3, const float *lambda4,
                       float *wi3, float *pdf_sample, float *Ls4, float *dist);
int avr_light_pick_at(avr_context *ctx, int n, const float *u, const float *p3, int *idx, float *pmf);
int avr_light_bvh(avr_context *ctx, int *n_nodes, float *phi, float *w3, int *qcos, int *qb, int *link, int *leaf,
                  float all_bounds[6], int *n_infinite);

/* Camera: type 0 orthographic, 1 perspective (cameras.cpp:284-306, 404-427).
 * camera_from_raster: full 4x4 (projective for perspective); render_from_camera: affine 4x4. */
int avr_camera(avr_context *ctx, int type, const float camera_from_raster[16], const float render_from_camera[16]);

/* The projective cameras' thin lens (lensradius / focaldistance, cameras.cpp:292-303, 413-424):
 * call after avr_camera, which resets to the pinhole; radius 0 is the pinhole. The lens sample is
 * GetCameraSample's (sampler dimensions 4 and 5). AVR_ERR_ARG: a negative or non-finite radius, a
 * focal distance <= 0 or NaN, a spherical camera; AVR_ERR_STATE: no camera yet. */
int avr_camera_lens(avr_context *ctx, float lens_radius, float focal_distance);

/* SphericalCamera (cameras.cpp:610-687) in place of avr_camera: mapping 0 equalarea, 1
 * equirectangular; uv = pFilm / the film's full resolution; render_from_camera: affine 4x4. */
int avr_camera_spherical(avr_context *ctx, int mapping, const float render_from_camera[16]);

/* RGBFilm with a box filter and a PixelSensor (film.h:95-100, 232-316): sensor_rgb is the
 * 3 x 471 r̄ḡb̄ (cie1931: X, Y, Z) tables, imaging_ratio = exposureTime*ISO/100.
 * Allocates and zeroes the fp64 film sums (3 + 1 doubles per pixel). */
int avr_film(avr_context *ctx, int width, int height, const float filter_radius[2], const float *sensor_rgb,
             float imaging_ratio, float max_component_value);
int avr_film_clear(avr_context *ctx);
/* Film::pixelBounds (film.h:67; "cropwindow" / "pixelbounds", film.cpp:97-172): after avr_film,
 * whose width and height stay the full resolution, render only the pixels [x0, x1) x [y0, y1).
 * Samplers, pixel filter and camera keep taking the absolute pixel and the full resolution
 * (ZSobolSampler, samplers.h:228-238; ImageTileIntegrator::Render, cpu/integrators.cpp:109,170),
 * so the bounds' pixels receive, sample for sample, what they receive in a render of the whole
 * film. Everything this header sizes by "W*H" is from then on sized by the bounds' pixel count
 * (x1-x0)*(y1-y0), row-major within the bounds: the film sums and every readback of them, the
 * per-sample records of the avr_last_pass_* and graph readbacks, images, references and metrics,
 * the export buffer and the pixel order. The call reallocates and zeroes the sums (a
 * SpectralFilm's buckets too, in whichever order avr_film_spectral and this call come) and drops
 * the pixel order, the analysis sums, the metric reference and whatever was built ahead for the
 * old bounds. avr_film resets the bounds to the whole film. Bounds that are empty or reach
 * outside the film: AVR_ERR_ARG (clamping is the caller's, as it is Film::Create's in pbrt);
 * before avr_film: AVR_ERR_STATE. */
int avr_film_pixel_bounds(avr_context *ctx, int x0, int y0, int x1, int y1);
int avr_film_get_bounds(avr_context *ctx, int *x0, int *y0, int *x1, int *y1);
/* Pixel filter for later renders (GetCameraSample, samplers.h:797-815): type 0 BoxFilter
 * (filters.h:48-77, radius), 1 GaussianFilter(radius, sigma) (filters.h:80-118; sampled with
 * FilterSampler's tabulated distribution, filters.cpp:133-147, weight f/pdf; radius <= 4).
 * pbrt's default filter is gaussian radius 1.5, sigma 0.5 (scene.cpp:94, filters.cpp). */
int avr_set_filter(avr_context *ctx, int type, const float radius[2], float sigma);
/* Pixel sampler for later renders: 0 IndependentSampler (samplers.h:442-476, default here),
 * 1 ZSobolSampler with FastOwen randomisation (samplers.h:225-330; pbrt's default,
 * scene.cpp:93). samples_per_pixel is the sampler's pixelsamples: ZSobol lays out
 * (Morton(pixel) << log2(spp)) | sampleIndex, so avr_render must stay below it. */
int avr_set_sampler(avr_context *ctx, int kind, int samples_per_pixel);
/* ZSobolSampler: GetSampleIndex's digits above log2(spp) depend on (pixel, dimension) only;
 * the first render after a sampler/film change tabulates them for the first `dims`
 * dimensions (4 B per pixel-Morton row and dimension; default 256, 0 = compute every digit
 * per call). Results are identical either way. */
int avr_set_sampler_table(avr_context *ctx, int dims);
/* ZSobolSampler in the persistent kernel: a pass renders sample indices [b, b + S) that agree
 * above their lowest L differing bits, so every digit of GetSampleIndex above them — and the
 * permutation of the one just below, whose hash reads only those bits — is shared by the
 * pass's samples of one pixel. Each pass tabulates them for the first `dims` dimensions
 * (8 B per pixel-Morton row and dimension; default 96, 0 = off) and a sampler call then
 * evaluates only the digits below (2 base-4 digits for 64-index passes instead of
 * log2(spp)/2). Results are identical either way. Odd `dims` are rounded up to even (rows
 * of 16-B aligned entry pairs). Memory: two tables of rows x dims x 8 B (the pass's and the
 * level-A table it is derived from), rows = Morton(width - 1, height - 1) + 1 — 1.64 M rows at
 * 720p, 1.26 GB per table at 96 dimensions, up to ~4x the pixel count for non-square films —
 * allocated lazily by the first render, only with >= 8 GiB of HBM to spare (else the pixel
 * table serves every draw), next to max_paths' records; with dims >= 10 also a 48-B per-pixel
 * copy of the camera stage's six entries (44 MB at 720p). */
int avr_set_sampler_pass_table(avr_context *ctx, int dims);

/* Render sample indices [spp_begin, spp_end) of every pixel (the avr_set_sampler sampler,
 * seed), VolPathIntegrator maxdepth. Asynchronous on the context stream. */
int avr_render(avr_context *ctx, int spp_begin, int spp_end, int seed, int max_depth);
/* Integrator::Tr (cpu/integrators.cpp:324-374): ratio-tracking transmittance from p0[i] to
 * p1[i] (render space, xyz) at the four wavelengths lambda[4i..4i+3] (nm), n queries; writes
 * tr[4i..4i+3] = Tr / inv_w.Average(). RNG per query seeded with Hash(p0), Hash(p1), as pbrt.
 * avr_transmittance: host arrays, synchronous. _device: device arrays, async on the stream. */
int avr_transmittance(avr_context *ctx, long long n, const float *p0, const float *p1, const float *lambda,
                      float *tr);
int avr_transmittance_device(avr_context *ctx, long long n, const float *p0, const float *p1, const float *lambda,
                             float *tr);
/* Waits for the context's stream and for its side stream (work built ahead for a next pass). */
int avr_sync(avr_context *ctx);
int avr_get_stats(avr_context *ctx, avr_stats *out);   /* waits for queued work */
int avr_reset_stats(avr_context *ctx);

/* Film readback: rgb_sum[W*H*3] and w_sum[W*H] (fp64 RGBFilm::Pixel sums). */
int avr_film_read(avr_context *ctx, double *rgb_sum, double *w_sum);
/* SpectralFilm (film.h:401-530; SpectralFilm::Create film.cpp:1037-1066 "nbuckets",
 * "lambdamin", "lambdamax"): after avr_film, n_buckets > 0 switches the film to uniform
 * wavelength sampling (SampledWavelengths::SampleUniform) over [lambda_min, lambda_max]
 * (within 360..830 nm here) and per-pixel bucket sums next to the RGB sums
 * (SpectralFilm::AddSample, film.h:413-455); 0 returns to RGBFilm. Readback: the fp64
 * Pixel::bucketSums / weightSums, [pixel * n_buckets + bucket]. */
int avr_film_spectral(avr_context *ctx, int n_buckets, float lambda_min, float lambda_max);
int avr_film_read_spectral(avr_context *ctx, double *bucket_sums, double *weight_sums);
int avr_film_spectral_device_ptrs(avr_context *ctx, void **d_bucket_sums, void **d_weight_sums);
/* In-process multi-GPU render (one context per GPU, e.g. avr_render(ctx_k, k*spp/N,
 * (k+1)*spp/N, ...)): SUM-reduce the n contexts' film sums (rgb, weights, SpectralFilm
 * buckets) into ctxs[root]'s film over RCCL (xGMI); the other films are left as they are.
 * Films must match in resolution and buckets; one context per device. The communicators
 * are created on the first reduce of a context list (ncclCommInitAll) and cached on the
 * contexts for later reduces of the same list; avr_context_destroy releases them.
 * Threading: the cached communicators tie the listed contexts together. Destroying one of
 * them, or reducing over a different list that contains one of them, destroys the whole
 * group's communicators; neither may run while another thread renders, reduces or reads on
 * any context of that group (calls on one context are serialized by the caller anyway). */
int avr_film_reduce_rccl(avr_context **ctxs, int n, int root);
/* Device pointers of the film sums (for an RCCL reduce across GPUs). */
int avr_film_device_ptrs(avr_context *ctx, void **d_rgb_sum, void **d_w_sum);
/* Device-to-device copy of the film sums into caller memory on the same GPU, laid out
 * [rgb_sum (W*H*3) | w_sum (W*H)] as doubles — the buffer handed to the RCCL reduce; a
 * SpectralFilm appends [bucket_sums (W*H*nb) | weight_sums (W*H*nb)]. */
int avr_film_export_device(avr_context *ctx, void *d_dst);

/* RGBFilm::GetImage on the device (film.cpp:533-565): per pixel GetPixelRGB (film.h:258-274)
 * with the caller's outputRGBFromSensorRGB (row-major 3x3), optionally as the fp16 image
 * ("savefp16": clamp to 65504, round to half). d_out: W*H*3 floats on this GPU. */
int avr_film_image_device(avr_context *ctx, const float output_from_sensor[9], int fp16, float *d_out);
/* --mse-reference-image (integrators.cpp:119-148, 209-219): keep a W*H*3 reference image
 * (host, row-major RGB) on the device; avr_film_metric then compares the film's GetImage
 * with it: metric 0 MSE, 1 MAE, 2 MRSE -> 3 per-channel values; 3 ME -> 9 values
 * (absolute, positive, negative per channel) with Image::MSE/MAE/MRSE/ME's definitions
 * (util/image.cpp:543-678), f64 sums by a fixed-order device reduction. */
int avr_film_set_reference(avr_context *ctx, const float *reference_rgb, const float output_from_sensor[9],
                           int fp16);
int avr_film_metric(avr_context *ctx, int metric, float *out);

/* FLIP error map (src/ext/flip/flip.cpp ComputeFLIPError, used by `imgtool diff --metric
 * FLIP`): test and reference are width*height RGB (interleaved, row-major) sRGB-encoded
 * values as the caller passes them (imgtool clamps to [0,1] first); ppd <= 0 takes the
 * reference's default 0.7 m / 0.7 m / 3840 px monitor. error: width*height floats. */
int avr_flip(avr_context *ctx, const float *test_rgb, const float *reference_rgb, int width, int height, float ppd,
             float *error);

/* ---- Lighting graph (src/graph/, the fork's own SampleT_maj callers) ----
 * The medium is the context's (avr_medium_*); geometry model: the medium's bounds box is
 * the boundary primitive. Sampling follows the reference's graph tools
 * (cmd/graph_maker.cpp:97-104): the scene sampler at its film resolution with
 * Options->pixelSamples, sampling index i -> pixel (i % resolution_x, i / resolution_x)
 * (graph/util.h:816-817).
 * The primitive of the geometry model is chosen per context with avr_graph_set_geometry: the
 * bounds box (the default) or the medium's interface. avr_graph_start_rays,
 * avr_graph_walks[_from], avr_graph_reinforce_rays, avr_graph_light, avr_graph_render and
 * avr_graph_analyze all follow it. bounds_center and max_dist_to_center (avr_graph_start_rays,
 * avr_graph_light) are the caller's, from the bounds of that primitive (PrimitiveData,
 * graph/util.h:45-59: bounds centre and |Diagonal / 2|). */
typedef struct avr_graph_sampling {
    int sampler;             /* 0 IndependentSampler, 1 ZSobolSampler                     */
    int seed;                /* sampler seed (Options->seed)                              */
    int samples_per_pixel;   /* Options->pixelSamples (RoundUpPow2(lightIterations))      */
    int film_width, film_height; /* the sampler's full resolution (ZSobol Morton layout)  */
    int resolution_x;        /* Options->graph.samplingResolution.x                       */
} avr_graph_sampling;

/* The graph tools' primitive for this context: geometry 0 = the medium's bounds box (the
 * default), 1 = the medium's interface: the sphere of avr_medium_boundary_sphere, the convex
 * polyhedron of avr_medium_boundary_convex, or, with neither set, the bounds box with exactly
 * geometry 0's results. Every hit is one solve from the ray's own origin (GetHits, util.h:
 * 419-458): OutsideTwoHits {t0, t1} starts the ray at o + d t0 with tMax = t1 - t0,
 * InsideOneHit {exit} tracks from o to the exit, no hit sees no medium; no surface offset.
 * SampleT_maj still clips to the medium's bounds box, so an interface may stick out of it.
 * Any other value: AVR_ERR_ARG. The setting persists across avr_medium_* calls. */
int avr_graph_set_geometry(avr_context *ctx, int geometry);

/* FreeGraphBuilder::BuildGraph's ray grid (free/free_graph_builder.cpp:143-199): steps x steps
 * rays along in_dir, ray r = (x - 1) * steps + (y - 1) for x, y in 1..steps, from the grid
 * point ((corner + xv * step * x) + yv * step * y) with (xv, yv) = CoordinateSystem(in_dir),
 * corner = bounds_center - in_dir * max_dist_to_center * 2 - (xv + yv) * max_dist_to_center
 * and step = max_dist_to_center * 2 / (steps + 1). Per ray: type (0 OutsideTwoHits, 2
 * OutsideZeroHits, 3 InsideOneHit: the primitive's GetHits), o (r*3: the origin after
 * SkipIntersection; the grid point when the ray misses) and t_first (the first segment's
 * tMax; 0 on a miss). The sampling index of ray r's first walk is r * iterationsPerStep.
 * steps: 0..32768 (0 does nothing). Host arrays, synchronous. */
int avr_graph_start_rays(avr_context *ctx, const float bounds_center[3], float max_dist_to_center,
                         const float in_dir[3], int steps, int *type, float *o, float *t_first);

/* FreeGraphBuilder::TracePath (free/free_graph_builder.cpp:19-141), the medium walk: for
 * each of n_rays rays (origin o, direction d, first segment end t_first = the medium exit
 * after SkipIntersection, BuildGraph :166-196) `iterations` walks, walk w = ray*iterations+i
 * started with StartPixelSample(pixel(index0[ray] + i), sample_index). Writes up to
 * max_depth scatter points per walk to points[(w*max_depth + k)*3 ..] and the count to
 * counts[w] (count == max_depth: the reference's forcedEnd). Host arrays, synchronous. */
int avr_graph_walks(avr_context *ctx, const avr_graph_sampling *smp, long long n_rays, const float *o, const float *d,
                    const float *t_first, const long long *index0, int iterations, int sample_index, int max_depth,
                    float *points, int *counts);

/* avr_graph_walks with skip_dims sampler dimensions drawn after StartPixelSample before the
 * walk (the reinforcement walks continue the stream their ray's phase sample started). */
int avr_graph_walks_from(avr_context *ctx, const avr_graph_sampling *smp, long long n_rays, const float *o,
                         const float *d, const float *t_first, const long long *index0, int iterations,
                         int sample_index, int skip_dims, int max_depth, float *points, int *counts);

/* FreeGraphBuilder::ReinforceSparseVertices' rays (free_graph_builder.cpp:434-475): for each of
 * n vertices (ids, points n*3), GetSphereVolumePointsRandom(vertex_radius, point, n_rays) with
 * the sampler at StartPixelSample({0, 0}, cycle), then per sphere point p the medium's HG
 * Sample_p((1,0,0), Get2D()) at StartPixelSample(pixel(id * n_rays + p), cycle) and the
 * primitive's crossing (avr_graph_set_geometry; the medium box by default): o/d (n*n_rays*3), t_first (medium exit after SkipIntersection), valid
 * (RayEntersVolume). The walk from each valid ray: avr_graph_walks_from(.., index0 =
 * id * n_rays + p, iterations 1, sample_index cycle, skip_dims 2, max_depth - 1). */
int avr_graph_reinforce_rays(avr_context *ctx, const avr_graph_sampling *smp, int n, const int *vertex_ids,
                             const float *points, float vertex_radius, int n_rays, int cycle, float *o, float *d,
                             float *t_first, int *valid);

/* LightingCalculator::GetLightVector (lighting_calculator.cpp:84-155) with
 * ComputeRaysToSphere (graph/util.h:814-840) and SampleTransmittance (util.h:344-366):
 * light[v] = Inv4Pi * average over the disk points of vertex v (GetDiskPoints(vertex -
 * in_dir * max_dist_to_center * 2, sphere_radius, points_on_radius, in_dir)) whose ray along
 * in_dir crosses the primitive (avr_graph_set_geometry; the medium box by default) and the
 * vertex's sphere inside it, of the average of
 * `iterations` ratio-tracking transmittances to a uniform point of the sphere chord.
 * vertices: n_vertices*3 (ids 0..n-1 in order). Host arrays, synchronous. */
int avr_graph_light(avr_context *ctx, const avr_graph_sampling *smp, int n_vertices, const float *vertices,
                    const float in_dir[3], float sphere_radius, int points_on_radius, int iterations,
                    float max_dist_to_center, float *light);

/* LightingCalculator::ComputeFinalLight (lighting_calculator.cpp:23-59): total = light +
 * sum of T^k light for k = 1..bounces, T in CSR (row_ptr[n+1], col ascending per row, val),
 * stopping before the first bounce whose vector holds a NaN/Inf; *iterations = bounces
 * completed. _device: device arrays, async on the context's stream (iterations read back
 * synchronously when non-null). */
int avr_graph_propagate(avr_context *ctx, int n, const int *row_ptr, const int *col, const float *val,
                        const float *light, int bounces, float *total, int *iterations);
int avr_graph_propagate_device(avr_context *ctx, int n, long long nnz, const int *row_ptr, const int *col,
                               const float *val, const float *light, int bounces, float *total, int *iterations);

/* FreeGraph assembly on the host (free_graph_builder.cpp:100-131, graph.cpp:134-229):
 * walks merged in walk order into vertices of radius `vertex_radius` — a scatter point joins
 * the nearest vertex strictly within the radius (nanoflann's RadiusResultSet bound; the
 * reference takes the first one its kd-tree reports), else the path's previous vertex when
 * within the radius, else becomes a new vertex; consecutive path vertices add edge samples;
 * each traced segment after a scatter counts a sample of the path's last vertex
 * (HandlePotentialPathEnd). avr_graph_transport: GetTransportMatrix (:61-82) as CSR rows
 * (row = vertex, col ascending, val = edge samples / vertex samples); row_ptr n+1, col/val
 * n_edges entries. */
typedef struct avr_graph avr_graph;
int avr_graph_create(float vertex_radius, avr_graph **out);
int avr_graph_destroy(avr_graph *g);
int avr_graph_add_walks(avr_graph *g, long long n_walks, int max_depth, const float *points, const int *counts);
/* Walks that start at an existing vertex (TracePath's startingVertex; -1 = none), traced with
 * max_depth - 1 scatters when a start vertex is given (max_depth counts path vertices). */
int avr_graph_add_walks_from(avr_graph *g, long long n_walks, int max_depth, const float *points, const int *counts,
                             const int *start_vertex);
/* The merge in data-parallel rounds (csrc/avr_graph_merge.h): which vertex every scatter
 * point of a batch of walks belongs to, exactly as avr_graph_add_walks_from would decide it in
 * walk order. Walks as there: points n_walks x max_depth x 3, counts, start_vertex per walk
 * or NULL (none). vertex_of_point: n_walks x max_depth ids, -1 past a walk's count; an id
 * equal to the number of vertices that exist at the point's turn (the graph's, plus the new
 * ones before it in walk, then point order) means the point becomes that new vertex.
 * avr_graph_merge_assign runs synchronous rounds on the host, avr_graph_merge_assign_device one
 * kernel sweep per round over the points still open (states read while other lanes write
 * them, so it needs at most the host's rounds); both leave the graph untouched, sort the
 * call's entities on the host, and give the same ids. *rounds (may be NULL): rounds run.
 * AVR_ERR_INTERNAL instead of looping if a round finalises no point (a bug: the open point of
 * lowest sequence can always be finalised). AVR_ERR_ARG: counts or start vertices out of range
 * as avr_graph_add_walks_from checks them, a non-finite coordinate, null buffers. Empty
 * batches and walks of count 0 are valid.
 * avr_graph_add_walks_assigned: avr_graph_add_walks_from with the radius search replaced by
 * vertex_of_point (vertex samples, edges in first-seen order and the in-node path lengths
 * follow in O(points)); AVR_ERR_ARG with the graph unchanged for a negative id or one above the
 * vertex count at its turn. avr_graph_add_walks_device: avr_graph_merge_assign_device, then the
 * replay; stats (may be NULL): wall-clock milliseconds of the host sort and upload, of the
 * device rounds with the id scan and its download, and of the replay. */
typedef struct avr_graph_merge_stats {
    int rounds;
    long long points;         /* scatter points in the call            */
    long long new_vertices;   /* of them, points that became vertices  */
    double ms_sort, ms_rounds, ms_replay;
} avr_graph_merge_stats;
int avr_graph_merge_assign(const avr_graph *g, long long n_walks, int max_depth, const float *points, const int *counts,
                           const int *start_vertex, int *vertex_of_point, int *rounds);
int avr_graph_merge_assign_device(avr_context *ctx, const avr_graph *g, long long n_walks, int max_depth,
                                  const float *points, const int *counts, const int *start_vertex, int *vertex_of_point,
                                  int *rounds);
int avr_graph_add_walks_assigned(avr_graph *g, long long n_walks, int max_depth, const float *points, const int *counts,
                                 const int *start_vertex, const int *vertex_of_point);
int avr_graph_add_walks_device(avr_context *ctx, avr_graph *g, long long n_walks, int max_depth, const float *points,
                               const int *counts, const int *start_vertex, avr_graph_merge_stats *stats);
/* Vertex::outEdges.size() per vertex; CountInRadius (squared distance < radius^2, self included) */
int avr_graph_out_degrees(avr_graph *g, int *out);
int avr_graph_count_in_radius(avr_graph *g, int n, const int *vertex_ids, float radius, int *counts);
int avr_graph_size(avr_graph *g, long long *n_vertices, long long *n_edges);
int avr_graph_vertices(avr_graph *g, float *xyz, int *samples);
int avr_graph_edges(avr_graph *g, int *from, int *to, int *samples);
int avr_graph_transport(avr_graph *g, int *row_ptr, int *col, float *val);
/* UseAndRemovePathInfo's in-node path length average (free_graph_builder.cpp:241-273) */
int avr_graph_in_node_path_length(avr_graph *g, float *average, long long *count);

/* The graph render's vertex index (GraphIntegrator::Initialize, graph_integrator.cpp:50-80:
 * squared vertex radius, squared search ranges with their 99th percentile
 * sorted[n * 99 / 100] and maximum, the search structure). Host code, no GPU needed. n
 * vertices (id = row of xyz, n*3), their VertexData::lightScalar, and their
 * renderSearchRange or NULL (streamFlags->useRenderSearchRange = false). Layout: a uniform
 * cell grid over the vertices' bounding box, vertices counting-sorted by cell, one 16-B record
 * {x, y, z, lightScalar} each; cell edge = vertex_radius, doubled until the grid holds at most
 * 2^21 cells. AVR_ERR_ARG: n < 1, a radius that is not positive and finite, a non-finite
 * coordinate, a negative or non-finite search range.
 * avr_graph_index_connect: ConnectToGraph (:249-280) for n points already in graph space.
 * Distance d2 = ((qx-vx)^2 + (qy-vy)^2) + (qz-vz)^2 in float (nanoflann L2_Simple_Adaptor); a
 * vertex is in the result iff d2 < r2, strictly. Stage 0: r2 = Sqr(vertex_radius). With search
 * ranges and an empty stage 0: stage 1, r2 = the 99th-percentile squared range, dropping
 * vertices with d2 > Sqr(range[v]); if still empty stage 2, r2 = the largest squared range,
 * same filter. Result in ascending d2 (nanoflann sorts; ties, unspecified there, go to the
 * lower vertex id), then Averager (graph/util.h:529-568): average += light * (1 / d2),
 * total += 1 / d2, in float in that order, for any number of neighbours; empty or total == 0
 * gives 0, d2 == 0 the reference's infinite weight and NaN. count_out: vertices averaged.
 * Points outside the grid's box and radii beyond it are handled. */
typedef struct avr_graph_index avr_graph_index;
int avr_graph_index_create(long long n, const float *xyz, const float *light_scalar, const float *search_range,
                           float vertex_radius, avr_graph_index **out);
int avr_graph_index_destroy(avr_graph_index *idx);
int avr_graph_index_connect(const avr_graph_index *idx, long long n, const float *points, float *light_out,
                            int *count_out);
/* avr_graph_index_connect on the device: the same search routine, one lane per point, with
 * bitwise the host's results. The index is uploaded on first use and cached on the context
 * under an id stored in the index (not its address); the copy is released with the context
 * or when another index is used. Host arrays, synchronous. */
int avr_graph_connect(avr_context *ctx, const avr_graph_index *idx, long long n, const float *points,
                      float *light_out, int *count_out);
/* FreeGraphBuilder::GetNClosest and ComputeSearchRanges (free_graph_builder.cpp:473-548) over
 * the index; host code, no GPU needed (the index's light scalars and ranges play no part).
 * avr_graph_index_knn: per vertex its k nearest other vertices, row = vertex id, k entries
 * each of ids and d2, in ascending key (d2, id); d2 = ((dx^2 + dy^2) + dz^2) in float as above.
 * The reference asks nanoflann for k + 1, sorts and drops item 0 (the vertex itself); here the
 * vertex is left out by id, the same unless another vertex coincides with it exactly, and
 * equal distances, which nanoflann leaves unspecified, go to the lower id. The search radius
 * starts at the cell edge and doubles until k + 1 vertices lie strictly inside it, for
 * isolated vertices and radii beyond the grid too. ids or d2 may be NULL where only the other
 * is wanted. A neighbour whose float d2 overflows is not found (id -1, d2 +inf).
 * avr_graph_index_search_ranges: renderSearchRange per vertex id (n floats) from two
 * Averager levels (graph/util.h:551-568) in float: avg[v] = the sum from 0 of sqrtf(d2[v][i]),
 * i ascending, over (float)k; range[v] = (avg[v] + avg[nb[v][0]] + ... + avg[nb[v][k-1]]),
 * summed in that order from 0, over (float)(k + 1).
 * AVR_ERR_ARG: k < 1, k > 15 (the sorted buffer holds 16 keys, the vertex included),
 * k > n - 1, null buffers. The reference accepts k == n and then reads neighbours[-1];
 * refusing it is a deviation. */
int avr_graph_index_knn(const avr_graph_index *idx, int k, int *ids, float *d2);
int avr_graph_index_search_ranges(const avr_graph_index *idx, int k, float *ranges);
/* The same on the device (k_graph_knn: one lane per sorted vertex, the sorted buffer in LDS;
 * k_graph_range_average: one lane per vertex), with bitwise the host's results. Reuses the
 * context's cached copy of the index as avr_graph_connect does. Host arrays, synchronous.
 * Kernel times: k_graph_knn adds to avr_stats ms_medium, k_graph_range_average to ms_film. */
int avr_graph_knn(avr_context *ctx, const avr_graph_index *idx, int k, int *ids, float *d2);
int avr_graph_search_ranges(avr_context *ctx, const avr_graph_index *idx, int k, float *ranges);
/* GraphIntegrator::Li, free-graph branch (graph_integrator.cpp:180-247), for sample indices
 * [spp_begin, spp_end) of every pixel, added to the film: avr_render's wavefront pass loop
 * (k_camera, then k_graph_render instead of the path kernels, then k_film; passes of at most
 * max_paths samples). Per sample: the camera ray (as the camera generates it, not moved to an
 * interface) crosses the primitive of avr_graph_set_geometry, the medium's bounds box by
 * default (the graph tools' geometry model, DESIGN.md §9: a ray from outside starts at its
 * entry point and ends at the exit; a camera inside, commented out in the reference, tracks from its
 * origin; a miss gives L = 0), RNG(Hash(Get1D), Hash(Get1D)), SampleT_maj with the next Get1D
 * and the medium's coefficients at the sample's own wavelengths, the 3-way event choice on
 * channel 0; the first real scatter p gives L = lightSpectrum.Sample(lambda) *
 * ConnectToGraph(graph_from_render(p)), lightSpectrum = the distant light's scale * Lemit;
 * absorption or leaving the primitive L = 0. graph_from_render: row-major affine 4x4 (the
 * reference's worldFromRender for a graph in world space), NULL = identity (the graph tools
 * here work in render space). Requires medium, camera and film, exactly one light of type 0
 * and, while the context's graph geometry is 0, no interface sphere / convex (AVR_ERR_STATE
 * otherwise; avr_graph_set_geometry(ctx, 1) takes the interface); sample-range and ZSobol limits
 * as avr_render. Work counters: the avr_stats fields avr_graph_walks uses (shadow_lookups,
 * shadow_items, shadow_dda_steps); the kernel's time in ms_medium. */
int avr_graph_render(avr_context *ctx, const avr_graph_index *idx, const float graph_from_render[16], int spp_begin,
                     int spp_end, int seed);
/* The last pass of the last avr_graph_render, indexed as avr_last_pass_samples (which, with
 * avr_last_pass_weights, returns that pass's L, wavelengths, pdfs and filter weights): the
 * camera ray o, d (n*3 each), the scatter point in render space (n*3) and the number of
 * vertices averaged, -1 when the sample did not scatter. Any output may be NULL.
 * After avr_graph_render_uniform with view 0: the scatter point in render space and 1 (its
 * voxel has a vertex), 0 (scattered, no vertex) or -1 (no scatter); with view 1: the point
 * `middle` in graph space and 1 / 0 (a lit voxel was hit, and the lookup at middle found /
 * did not find a vertex), -1 otherwise.
 * AVR_ERR_STATE when the last render was avr_render's or avr_graph_analyze's. */
int avr_graph_last_pass(avr_context *ctx, float *o, float *d, float *points, int *counts, long long n_max);

/* The uniform (voxel) lighting graph: UniformGraph (graph/graph.h:195, graph.cpp:545-577),
 * vertices on the integer lattice of a spacing. Host code, no GPU needed.
 * Coordinates (FitToGraph, graph/util.h:302-311): per axis q = p / spacing in float, r =
 * roundf(q) (half away from zero), c = (int)r; valid iff |r| < 2^20 (the reference casts any
 * value; NaN is invalid), so that a voxel packs into one 64-bit key. The vertex's point is
 * (float)c * spacing per axis. Lookup structure: one open-addressing hash table with linear
 * probing, 16-B entries {key, id, lightScalar}, capacity the smallest power of two >= 2 m (at
 * least 16), uploaded to the device on first use and cached on the context under an id stored
 * in the object, as avr_graph_index is.
 * avr_graph_uniform_create: m vertices with coordinates coors (m*3) and lightScalar light (m);
 * AVR_ERR_ARG, naming the vertex: spacing not finite or <= 0, m < 1, a coordinate outside
 * +-2^20, a NaN light, a repeated coordinate.
 * avr_graph_uniform_from_points: FreeGraph::ToUniform's vertex part (graph.cpp:597-604,
 * 545-564) for n free-graph vertices xyz (n*3) with lights light (n). The vertices are taken
 * in ascending id (the reference iterates an unordered map: its order is unspecified) and a
 * new vertex is made at the first appearance of a voxel, new ids in that order. reduce 0
 * ("first"): the voxel keeps its first vertex's light (AddVertex returns the existing vertex);
 * reduce 1 ("mean"): the float sum from 0 of its vertices' lights in ascending id over
 * (float)count. vertex_of (n, may be NULL): old -> new id. Edges and paths are not carried.
 * AVR_ERR_ARG as above, and for a point whose coordinate is invalid.
 * avr_graph_uniform_get: the coordinates (m*3) and lights (m) by vertex id; either may be NULL.
 * avr_graph_uniform_lookup: UniformGraph::GetVertexConst for n points in graph space: the
 * vertex id of the point's voxel or -1 (also for an invalid coordinate) and its light (0
 * without a vertex). Either output may be NULL.
 * avr_graph_uniform_trace: --graph-debug's search (graph_integrator.cpp:104-131) for n rays
 * o + t d (n*3 each) in graph space: among the vertices with light != 0, the one whose box
 * [mid - spacing / 2, mid + spacing / 2] the ray enters first, with hit0 and hit1 of
 * Bounds3::IntersectP(o, d, Infinity, &hit0, &hit1) for it (t0 from 0, tFar widened by
 * 1 + 2 gamma(3)); id -1 and 0, 0 without one. The reference keeps the smallest hit0 over all
 * lit voxels with a strict < in unordered-map order; here equal hit0 go to the lower id. A
 * 3-D DDA over the lattice cells with the exact IntersectP per lit candidate: the brute-force
 * answer whenever the two smallest hit0 differ and the winner's chord is more than rounding. */
typedef struct avr_graph_uniform avr_graph_uniform;
int avr_graph_uniform_create(long long m, const int *coors, const float *light, float spacing, avr_graph_uniform **out);
int avr_graph_uniform_from_points(long long n, const float *xyz, const float *light, float spacing, int reduce,
                                  int *vertex_of, avr_graph_uniform **out);
int avr_graph_uniform_destroy(avr_graph_uniform *u);
int avr_graph_uniform_size(const avr_graph_uniform *u, long long *n_vertices, float *spacing);
int avr_graph_uniform_get(const avr_graph_uniform *u, int *coors, float *light);
int avr_graph_uniform_lookup(const avr_graph_uniform *u, long long n, const float *points, int *id_out,
                             float *light_out);
int avr_graph_uniform_trace(const avr_graph_uniform *u, long long n, const float *o, const float *d, int *id_out,
                            float *hit0, float *hit1);
/* The same on the device (k_graph_uniform_lookup, k_graph_uniform_trace: one lane per query)
 * with bitwise the host's results. Host arrays, synchronous; every output is required. */
int avr_graph_uniform_lookup_device(avr_context *ctx, const avr_graph_uniform *u, long long n, const float *points,
                                    int *id_out, float *light_out);
int avr_graph_uniform_trace_device(avr_context *ctx, const avr_graph_uniform *u, long long n, const float *o,
                                   const float *d, int *id_out, float *hit0, float *hit1);
/* GraphIntegrator::Li, uniform-graph branch (graph_integrator.cpp:89-178): avr_graph_render's
 * pass loop, requirements and errors with k_graph_render_uniform in place of k_graph_render.
 * view 0: the walk to the first real scatter p is avr_graph_render's, draw for draw; then
 * L = (lightSpectrum.Sample(lambda) * lightScalar) * light_scale for the vertex of
 * graph_from_render(p)'s voxel, 0 without one. The reference's light_scale is Inv4Pi; a
 * graph lit by avr_graph_light already carries Inv4Pi and takes 1. view 1, --graph-debug's
 * voxel view: no sampler draw and no tracking; the ray from where avr_graph_render's walk
 * starts, mapped to graph space (point and vector), finds its first lit voxel as
 * avr_graph_uniform_trace does; middle = o' + d' * ((hit0 + hit1) / 2); L =
 * lightSpectrum.Sample(lambda) * lightScalar of the vertex at middle (light_scale unused), 0
 * on a miss of the primitive, without a lit voxel or without a vertex at middle.
 * AVR_ERR_ARG: view outside {0, 1}, a light_scale that is not finite. */
int avr_graph_render_uniform(avr_context *ctx, const avr_graph_uniform *u, const float graph_from_render[16],
                             int spp_begin, int spp_end, int seed, int view, float light_scale);

/* The voxel boundary, graph::VoxelBoundary (graph/voxels/voxel_boundary.cpp): a medium to a
 * voxel set in three steps: capture, single layer, fill.
 *
 * avr_graph_capture: CaptureBoundary's ray bundles (:13-62) on the device (k_graph_capture, one
 * lane per ray). Bundle b has origin, dir, xvec, yvec (n_bundles*3 each, the caller's: the
 * reference takes origin on a sphere around the medium, dir = bounds_center - origin, not
 * normalised, and (xvec, yvec) = CoordinateSystem(dir) * step); its (2 num_steps + 1)^2 rays
 * are (i, j) in [-num_steps, num_steps]^2, i outer, from p = (origin + xvec * (float)i) + yvec
 * * (float)j along dir. Per ray GetHits(primitive) of avr_graph_set_geometry: a miss captures
 * nothing, and neither does a start inside the primitive (the reference skips to the exit hit;
 * no medium lies beyond it); a ray from outside moves to its entry (SkipIntersection, no
 * offset) and runs the medium's majorant DDA with dir as given (SampleRay does not normalise)
 * and tMax = Infinity; the first segment with sigma_t[0] * majorant != 0 (sigma_t at the
 * graph tools' defaultLambda) gives the point p + dir * tMin. out_points4: 4 floats per ray in
 * ray order (bundle, i, j): x, y, z and 1 for a captured point, zeros without one;
 * *n_captured: how many. Every medium type avr_graph_walks takes; AVR_ERR_STATE without a
 * medium; AVR_ERR_ARG: a null pointer, n_bundles < 1, num_steps < 0, more than 2^31 - 1 rays.
 * Host arrays, synchronous.
 *
 * avr_graph_uniform_count_device / avr_graph_uniform_from_points_device:
 * avr_graph_uniform_from_points(reduce 0, lights 0) for points on the device
 * (k_graph_uniform_insert: one lane per point inserts its voxel key into an open-addressing
 * set with a 64-bit compare-and-swap and keeps the key's lowest point index with an atomic
 * min, so the result does not depend on scheduling; ids by a scan in the order of first
 * appearance): the number of distinct voxels, and the graph with bitwise the host's
 * coordinates, ids and vertex_of (n, may be NULL). The host routine's AVR_ERR_ARG cases and
 * messages, the lowest invalid point named.
 *
 * avr_graph_voxels_*: the two floods (csrc/avr_graph_voxels.h). The state is one byte per cell
 * of the dense lattice over FitBounds (util.h:313-317): lo = FitToGraph(pmin) - 1, hi =
 * FitToGraph(pmax) + 1, inclusive, pmin / pmax the bounds of the medium's primitive; x fastest.
 * Bits: 1 boundary vertex, 2 outside (visited by the first flood), 4 cast, 8 single-layer
 * vertex, 16 filled. _create takes the m vertices' lattice coordinates (m*3); AVR_ERR_ARG for
 * a spacing that is not positive and finite, m < 1, more than 2^31 - 1 cells, a vertex
 * outside the bounds or repeated.
 * _single_layer, ToSingleLayerAndSaveCast (:122-181): a 6-neighbour flood from lo over the
 * cells that are not vertices; a visited cell with a vertex neighbour is cast, a vertex with a
 * visited neighbour is single-layer. The reference's three-set scheme is a level-synchronous
 * breadth-first search that visits each cell once; its numVisited is _visited's `visited`.
 * _fill, FillInside (:183-225): a 6-neighbour flood over every cell that is not cast, from the
 * single-layer vertex `start` (an index into _create's vertices), from the lowest one (-1) or
 * from all of them (-2); the reference starts from unordered_map::begin(), which is
 * unspecified. It runs the single layer first when that has not run (:184-186). AVR_ERR_ARG
 * for a start that is no single-layer vertex.
 * ctx NULL runs a flood on the host (plain breadth-first loops); with a context it runs on the
 * device, one launch per level over a frontier list (k_graph_voxels_level), the frontier count
 * read back per level, and leaves bytewise the host's state. levels (may be NULL): the levels
 * run. _state: lo, n (cells per axis) and the state bytes (capacity: the buffer's size; any
 * of the three may be NULL). _visited: the cells with bit 2, 4, 8 and 16 (each may be NULL). */
typedef struct avr_graph_voxels avr_graph_voxels;
int avr_graph_capture(avr_context *ctx, int n_bundles, const float *origin, const float *dir, const float *xvec,
                      const float *yvec, int num_steps, float *out_points4, long long *n_captured);
int avr_graph_uniform_count_device(avr_context *ctx, long long n, const float *xyz, float spacing, long long *count);
int avr_graph_uniform_from_points_device(avr_context *ctx, long long n, const float *xyz, float spacing,
                                         avr_graph_uniform **out, int *vertex_of);
int avr_graph_voxels_create(const float pmin[3], const float pmax[3], float spacing, long long m, const int *coors,
                            avr_graph_voxels **out);
int avr_graph_voxels_destroy(avr_graph_voxels *v);
int avr_graph_voxels_single_layer(avr_context *ctx, avr_graph_voxels *v, int *levels);
int avr_graph_voxels_fill(avr_context *ctx, avr_graph_voxels *v, int start, int *levels);
int avr_graph_voxels_state(const avr_graph_voxels *v, int lo[3], int n[3], unsigned char *state, long long capacity);
int avr_graph_voxels_visited(const avr_graph_voxels *v, long long *visited, long long *cast, long long *single_layer,
                             long long *filled);

/* IntegrationAnalyzer's Analyze (graph/analysis/integration_analyzer.cpp:56-83) for n points
 * already in graph space; host code, no GPU needed. node[i] = 1 when radiusSearch(point,
 * Sqr(vertex_radius)) returns a vertex (d2 < r2 strictly, d2 as avr_graph_index_connect's).
 * in_range[i]: the vertices of radiusSearch(point, the largest squared search range) left
 * after those with d2 > Sqr(range[v]) are dropped (stage 2's search and filter); non-zero
 * counts one search scatter. range_sum[i]: the float sum from 0 of sqrtf(d2) over them in
 * ascending (d2, id), nanoflann's result order with ties to the lower id; exact for any
 * count. The reference adds every distance of every sample to one float Averager; here the
 * sum is per point, so that it can be checked bit for bit. An index without search ranges
 * gives in_range = 0 and range_sum = 0 (the reference would search its unset
 * maxSquaredSearchRange). Any output may be NULL. */
int avr_graph_index_coverage(const avr_graph_index *idx, long long n, const float *points, int *node, int *in_range,
                             float *range_sum);
/* avr_graph_index_coverage on the device (k_graph_coverage, one lane per point) with bitwise
 * the host's results, over the context's cached copy of the index as avr_graph_connect's.
 * Host arrays, synchronous. */
int avr_graph_coverage(avr_context *ctx, const avr_graph_index *idx, long long n, const float *points, int *node,
                       int *in_range, float *range_sum);
/* IntegrationAnalyzer::AnalyzeRay (integration_analyzer.cpp:55-163) for sample indices
 * [spp_begin, spp_end) of every pixel: avr_graph_render's pass loop with k_graph_analyze in
 * place of k_graph_render and k_graph_analyze_reduce in place of k_film; the film is not
 * touched. Per sample the camera ray crosses the graph geometry's primitive as avr_graph_render's
 * does (a miss analyses nothing) and then walks on as avr_graph_walks' paths do: per segment
 * RNG(Hash(Get1D), Hash(Get1D)) and SampleT_maj with the next Get1D, coefficients at the
 * sample's own wavelengths, the 3-way event choice on channel 0; absorption and leaving the
 * medium end the path; each of the first max_depth real scatters p is analysed by
 * avr_graph_index_coverage(graph_from_render(p)) and followed by the HG Sample_p(-d, Get2D);
 * the path stops right after the max_depth-th (the reference's further draws reach no
 * result). Per pixel five sums grow, in sample-index then scatter order: scatters analysed,
 * those with node = 1, those with in_range > 0, in_range, and (double)range_sum added in
 * double, so that a sample range split into passes or calls gives the same bits. The
 * reference's figures for a pixel: node / total, search / total and range_sum / in_range
 * (its float Averager chain differs from the last by rounding only). Requires medium, camera
 * and film (no light) and no interface sphere / convex (AVR_ERR_STATE); max_depth < 0 or a
 * bad sample range: AVR_ERR_ARG; max_depth 0 analyses nothing. graph_from_render, sampler,
 * ZSobol limits and seeds as avr_graph_render. detail != 0 also keeps the last pass's
 * scatters (avr_graph_analyze_last_pass) in a buffer of pass samples x max_depth x 24 B,
 * allocated only then; AVR_ERR_ARG when it would exceed the wavefront path state's own bound,
 * max_paths x 252 B. Work counters and kernel time as avr_graph_render (ms_medium;
 * k_graph_analyze_reduce in ms_film). */
int avr_graph_analyze(avr_context *ctx, const avr_graph_index *idx, const float graph_from_render[16], int spp_begin,
                      int spp_end, int seed, int max_depth, int detail);
/* The per-pixel sums of the analyses since the last clear (W*H entries each, row-major; any
 * may be NULL): scatters analysed, node scatters, search scatters, vertices in range and the
 * sum of their distances. avr_graph_analysis_clear zeroes them; a new avr_film does too. */
int avr_graph_analysis_read(avr_context *ctx, unsigned long long *total, unsigned long long *node,
                            unsigned long long *search, unsigned long long *in_range, double *range_sum);
int avr_graph_analysis_clear(avr_context *ctx);
/* The last pass of the last avr_graph_analyze called with detail != 0, samples indexed as
 * avr_graph_last_pass: the camera ray o, d (n*3 each), counts (n, scatters analysed) and per
 * sample max_depth entries (the analysis' max_depth) of the scatter point in render space
 * (points, n*max_depth*3) and avr_graph_index_coverage's answer for it (node, in_range,
 * range_sum, n*max_depth each); entries past a sample's count are zero. Any output may be
 * NULL. AVR_ERR_STATE when the last render was not an analysis with detail. */
int avr_graph_analyze_last_pass(avr_context *ctx, float *o, float *d, int *counts, float *points, int *node,
                                int *in_range, float *range_sum, long long n_max, int max_depth);

/* Per-sample radiance of the LAST wavefront pass of the last avr_render (replay checks;
 * pbrt's --debugstart analogue, integrators.cpp:74-102). Element id = s*W*H + pixel,
 * s = sampleIndex - first sample of that pass. Writes n_max*4 floats into each of
 * L, lambda, pdf and returns the pass's first sample index and sample count. */
int avr_last_pass_samples(avr_context *ctx, float *L, float *lambda, float *pdf, long long n_max,
                          int *first_sample, int *n_samples);
/* Filter weights (CameraSample::filterWeight) of the last pass's samples, same indexing.
 * Both readbacks fail with AVR_ERR_STATE once the pixel order (avr_set_pixel_order, or a new
 * avr_film that drops it) changed after that render: its records are in the old slot order. */
int avr_last_pass_weights(avr_context *ctx, float *weight, long long n_max);
/* The camera stage's rays of the last PERSISTENT pass, same indexing and the same pixel-order
 * rule: the render-space origin after the medium-interface entry (o3, n*3), the direction (d3,
 * n*3) and the first segment's free-flight draw (u, n). Any output may be NULL. AVR_ERR_STATE
 * after a wavefront render, whose ray state the path itself consumes. */
int avr_last_pass_rays(avr_context *ctx, float *o3, float *d3, float *u, long long n_max);
/* Template arguments of the last k_paths instantiation avr_render launched, as
 * "k_paths<emissive, gray, sampler, medium, image, fast>" (sampler 0 independent, 2 / 3 ZSobol
 * with 32- / 64-bit indices; "" before the first persistent render): lets a profiler pass
 * (rocprofv3 kernel names) be matched to the configuration that was timed. NUL-terminated,
 * truncated to cap bytes. */
int avr_last_kernel(avr_context *ctx, char *buf, int cap);

#ifdef __cplusplus
}
#endif
#endif /* AVR_H */
