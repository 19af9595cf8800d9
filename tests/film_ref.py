"""A plain numpy restatement of pbrt's film stage — TEST INFRASTRUCTURE, the second opinion on
k_film, k_film_image, the host GetImage forms and the oracle's AddSample.

Written from the reference's film.h / film.cpp text, statement by statement; it shares no code
with the kernel (csrc/avr_kernels.hip) or the oracle (oracle/volpath_oracle.cpp). Every float
operation is one float32 numpy operation in pbrt's order (numpy fuses nothing); the pixel sums
are float64 additions of the float32 products in sample-index order, as `double += Float` is.

`film` is a scene.RGBFilm / SpectralFilm / GBufferFilm: sensor (3, 471) r̄ ḡ b̄ tables from
360 nm, imaging_ratio, max_component_value, output_from_sensor and, for a SpectralFilm,
nbuckets, lambdamin, lambdamax.
"""
import numpy as np

F32 = np.float32
LAMBDA_MIN = 360                     # DenselySampledSpectrum(lambda_min = Lambda_min), spectrum.h
CIE_Y_INTEGRAL = F32(106.856895)     # spectrum.h:38
N_SPECTRUM_SAMPLES = 4


def _f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def _lround(x):
    """std::lround of a float: nearest integer, halfway cases away from zero."""
    x = np.asarray(x, np.float64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def _sample_dense(table, lam):
    """DenselySampledSpectrum::Sample (spectrum.h:389-400): the table entry at the wavelength
    rounded to an integer (lround) minus the table's first wavelength, 0 outside the table."""
    table = _f32(table)
    off = _lround(lam) - LAMBDA_MIN
    inside = (off >= 0) & (off < table.size)
    return np.where(inside, table[np.clip(off, 0, table.size - 1)], F32(0)).astype(F32)


def _safe_div(a, b):
    """SafeDiv (spectrum.h:634-639): the quotient where the divisor is not 0, else 0."""
    with np.errstate(all="ignore"):
        return np.where(b != 0, a / np.where(b != 0, b, F32(1)), F32(0)).astype(F32)


def _average(v):
    """SampledSpectrum::Average (spectrum.h:256-261): the values added left to right, then
    divided by their count."""
    with np.errstate(all="ignore"):
        s = v[:, 0]
        for i in range(1, N_SPECTRUM_SAMPLES):
            s = (s + v[:, i]).astype(F32)
        return (s / F32(N_SPECTRUM_SAMPLES)).astype(F32)


def _max_list(*xs):
    """std::max({a, b, ...}) / std::max(m, v) chains: largest = first; if (largest < next)
    largest = next — a NaN operand compares false, so a NaN first stays and a later NaN is
    skipped. Elementwise over arrays."""
    m = xs[0]
    for x in xs[1:]:
        m = np.where(m < x, x, m)
    return m


def radiance_guard(film, L, lam, pdf):
    """RayIntegrator::EvaluatePixelSample's NaN / Inf guard in front of AddSample
    (cpu/integrators.cpp:272-282): L becomes 0 when it holds a NaN or its luminance is infinite;
    SampledSpectrum::y (spectrum.cpp:218-222) is the average of Y * L safely divided by the pdfs,
    over the CIE Y integral.
    The identity on records that already went through it. film.sensor[1] is Spectra::Y() for
    the cie1931 sensor, which is the only one the project has."""
    L, lam, pdf = _f32(L).reshape(-1, 4), _f32(lam).reshape(-1, 4), _f32(pdf).reshape(-1, 4)
    with np.errstate(all="ignore"):
        ys = _sample_dense(film.sensor[1], lam)
        y = (_average(_safe_div((ys * L).astype(F32), pdf)) / CIE_Y_INTEGRAL).astype(F32)
    bad = np.isnan(L).any(axis=1) | np.isinf(y)
    out = L.copy()
    out[bad] = 0
    return out


def sensor_rgb(film, L, lam, pdf):
    """PixelSensor::ToSensorRGB (film.h:95-100): L safely divided by the wavelength pdfs; per
    channel the average of the response table's samples times that, and the imaging ratio times
    the average last. (n, 3) float32, before any clamp."""
    L, lam, pdf = _f32(L).reshape(-1, 4), _f32(lam).reshape(-1, 4), _f32(pdf).reshape(-1, 4)
    ratio = F32(film.imaging_ratio)
    with np.errstate(all="ignore"):
        Ld = _safe_div(L, pdf)
        cols = [(ratio * _average((_sample_dense(film.sensor[c], lam) * Ld).astype(F32))).astype(F32)
                for c in range(3)]
    return np.stack(cols, axis=1)


def clamp_shares(film, L, lam, pdf):
    """Fractions of samples on which the sensor-RGB clamp (film.h:245-247) and the spectral L
    clamp (film.h:436-438) fire for this film's maxcomponentvalue."""
    rgb = sensor_rgb(film, L, lam, pdf)
    L = _f32(L).reshape(-1, 4)
    mcv = F32(film.max_component_value)
    m = _max_list(rgb[:, 0], rgb[:, 1], rgb[:, 2])
    lm = _max_list(L[:, 0], L[:, 1], L[:, 2], L[:, 3])
    return float(np.mean(m > mcv)), float(np.mean(lm > mcv))


def add_samples(film, L, lam, pdf, w, npix):
    """RGBFilm::AddSample (film.h:239-255) / SpectralFilm::AddSample (film.h:413-455) over
    per-sample records in the last-pass layout (sample-major, record s * npix + pix), samples of
    a pixel in sample-index order. Returns (rgb_sum (3 npix), w_sum (npix)) float64 and, for a
    SpectralFilm, also (bucket_sums, weight_sums), each (npix, nbuckets) float64."""
    L, lam, pdf = _f32(L).reshape(-1, 4), _f32(lam).reshape(-1, 4), _f32(pdf).reshape(-1, 4)
    w = _f32(w).reshape(-1)
    n = L.shape[0]
    if n % npix or not (len(lam) == len(pdf) == n) or len(w) < n:
        raise ValueError("records do not fill whole samples of npix pixels")
    w = w[:n]
    mcv = F32(film.max_component_value)
    nb = int(getattr(film, "nbuckets", 0))

    with np.errstate(all="ignore"):
        # film.h:242: sensor RGB
        rgb = sensor_rgb(film, L, lam, pdf)
        # film.h:245-247: the largest component; above the limit, every component times (limit / largest),
        # the quotient rounded to float first
        m = _max_list(rgb[:, 0], rgb[:, 1], rgb[:, 2])
        hit = m > mcv
        k = (mcv / m).astype(F32)
        rgb = np.where(hit[:, None], (rgb * k[:, None]).astype(F32), rgb)
        # film.h:252-254: the float product weight * component added to the double sum; the weight to its sum
        contrib = (w[:, None] * rgb).astype(F32).astype(np.float64)

        rgb_sum = np.zeros((npix, 3), np.float64)
        w_sum = np.zeros(npix, np.float64)
        for s in range(n // npix):
            rgb_sum += contrib[s * npix:(s + 1) * npix]
            w_sum += w[s * npix:(s + 1) * npix].astype(np.float64)
        if nb <= 0:
            return rgb_sum.reshape(-1), w_sum

        # film.h:436-438: the same clamp on the undivided L by its largest component (spectrum.h:249-254)
        lm = _max_list(L[:, 0], L[:, 1], L[:, 2], L[:, 3])
        hit = lm > mcv
        k = (mcv / lm).astype(F32)
        Ls = np.where(hit[:, None], (L * k[:, None]).astype(F32), L)
        # film.h:447: L times the float product of the weight and the CIE Y integral
        Ls = (Ls * (w * CIE_Y_INTEGRAL).astype(F32)[:, None]).astype(F32)
        # LambdaToBucket (film.h:500-504): the bucket count (as float) times the offset from the range's
        # start, divided by the range's width, truncated toward zero, clamped to the buckets
        lmin, lmax = F32(film.lambdamin), F32(film.lambdamax)
        t = ((F32(nb) * (lam - lmin).astype(F32)).astype(F32) / F32(lmax - lmin)).astype(F32)
        bucket = np.clip(np.trunc(t).astype(np.int64), 0, nb - 1)

        bucket_sums = np.zeros((npix, nb), np.float64)
        weight_sums = np.zeros((npix, nb), np.float64)
        rows = np.arange(npix)
        for s in range(n // npix):
            sl = slice(s * npix, (s + 1) * npix)
            for i in range(N_SPECTRUM_SAMPLES):   # one pixel per row: no index repeats within an update
                bucket_sums[rows, bucket[sl, i]] += Ls[sl, i].astype(np.float64)
                weight_sums[rows, bucket[sl, i]] += w[sl].astype(np.float64)
    return rgb_sum.reshape(-1), w_sum, bucket_sums, weight_sums


def _half(x):
    """Image::SetChannel on a Half image: round to nearest even, overflow to inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        return F32(np.float16(x))


def _pixel_rgb(film, rgb_sum, w_sum, p):
    """RGBFilm::GetPixelRGB (film.h:258-274) / SpectralFilm::GetPixelRGB (film.cpp:889-907) with
    zero splats: the sums rounded to float, divided by the weight sum when it is not 0, then the
    output matrix applied as a row-by-row accumulation from 0: ((0 + m0 r) + m1 g) + m2 b."""
    rgb = [F32(rgb_sum[3 * p + c]) for c in range(3)]
    weight = F32(w_sum[p])
    if weight != 0:
        rgb = [F32(v / weight) for v in rgb]
    rgb = [F32(np.float64(v) + 0.0) for v in rgb]    # film.h:267-268: the splat term, a double 0 here
    m = np.asarray(film.output_from_sensor, F32).reshape(3, 3)
    out = []
    for i in range(3):
        acc = F32(0)
        for j in range(3):
            acc = F32(acc + F32(m[i, j] * rgb[j]))
        out.append(acc)
    return out


def _gated_clamp(rgb):
    """The fp16 clamp of film.cpp:543-551 and 761-769: where the maximum of the three channels
    exceeds 65504, each channel above 65504 becomes 65504. The maximum is std::max over an
    initializer list, written out as the scalar loop it is (a NaN first operand stays, a
    later NaN is skipped)."""
    largest = rgb[0]
    for nxt in rgb[1:]:
        if largest < nxt:
            largest = nxt
    if largest > 65504:
        rgb = [F32(65504) if v > 65504 else v for v in rgb]
    return rgb


def get_image_rgb(film, rgb_sum, w_sum, fp16=True):
    """RGBFilm::GetImage (film.cpp:533-565): (H, W, 3) float32 holding what the Half (fp16) or
    Float image holds."""
    rgb_sum = np.asarray(rgb_sum, np.float64).reshape(-1)
    w_sum = np.asarray(w_sum, np.float64).reshape(-1)
    npix = film.width * film.height
    out = np.zeros((npix, 3), F32)
    with np.errstate(all="ignore"):
        for p in range(npix):
            rgb = _pixel_rgb(film, rgb_sum, w_sum, p)
            if fp16:
                rgb = [_half(v) for v in _gated_clamp(rgb)]
            out[p] = rgb
    return out.reshape(film.height, film.width, 3)


def get_image_gbuffer(film, rgb_sum, w_sum, fp16=True):
    """GBufferFilm::GetImage (film.cpp:688-803) with no splats and no visible surface: R G B
    with the same gated clamp (761-769); every other channel stays at its zero start (normals
    of length 0 are written as 0, the variance estimators are empty). (H, W, 25) float32, not
    yet rounded to half (the project's gbuffer_image leaves that to its writer)."""
    rgb_sum = np.asarray(rgb_sum, np.float64).reshape(-1)
    w_sum = np.asarray(w_sum, np.float64).reshape(-1)
    npix = film.width * film.height
    out = np.zeros((npix, 25), F32)
    with np.errstate(all="ignore"):
        for p in range(npix):
            rgb = _pixel_rgb(film, rgb_sum, w_sum, p)
            if fp16:
                rgb = _gated_clamp(rgb)
            out[p, :3] = rgb
    return out.reshape(film.height, film.width, 25)


def get_image_spectral(film, rgb_sum, w_sum, bucket_sums, weight_sums, fp16=True):
    """SpectralFilm::GetImage (film.cpp:961-1028) with no splats: each RGB channel above 65504
    clamped on its own (no gate on the maximum); a bucket is 0 unless its weight sum is > 0, else
    the double quotient of its sums rounded to float, clamped the same way for fp16.
    (H, W, 3 + nbuckets) float32, not yet rounded to half."""
    rgb_sum = np.asarray(rgb_sum, np.float64).reshape(-1)
    w_sum = np.asarray(w_sum, np.float64).reshape(-1)
    npix, nb = film.width * film.height, int(film.nbuckets)
    bs = np.asarray(bucket_sums, np.float64).reshape(npix, nb)
    bw = np.asarray(weight_sums, np.float64).reshape(npix, nb)
    out = np.zeros((npix, 3 + nb), F32)
    with np.errstate(all="ignore"):
        for p in range(npix):
            rgb = _pixel_rgb(film, rgb_sum, w_sum, p)
            if fp16:
                rgb = [F32(65504) if v > 65504 else v for v in rgb]
            out[p, :3] = rgb
            for i in range(nb):
                c = F32(0)
                if bw[p, i] > 0:
                    c = F32(bs[p, i] / bw[p, i] + 0.0)
                    if fp16 and c > 65504:
                        c = F32(65504)
                out[p, 3 + i] = c
    return out.reshape(film.height, film.width, 3 + nb)
