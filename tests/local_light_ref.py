"""PointLight, SpotLight and BVHLightSampler restated in numpy from the reference's text
(lights.h:223-230, 779-791; lights.cpp:164-173, 1360-1380; util/math.h:268-274;
lightsamplers.h:101-228, 266-327, 383-396; lightsamplers.cpp:109-238; lights.h:137-153;
util/vecmath.cpp:56-83; util/vecmath.h:1734-1829; util/sampling.h:79-113) — TEST INFRASTRUCTURE.

Independent of csrc/avr_local_light.h: written operation by operation from the formulas, with the
arithmetic type a parameter. T = float32 follows the reference's float order; T = float64 is the
same formulas in double, which measures the float32 rounding of a quantity (the quantised integers
of CompactLightBounds are integers in both). The sampling functions are vectorised over reference
points; the BVH build is scalar. `mut` names one deliberately wrong formula (test sensitivity)."""
import numpy as np

F32, F64 = np.float32, np.float64
ONE_MINUS_EPS = np.float32(1) - np.float32(2.0 ** -24)
N_BUCKETS = 12


def _t(T, v):
    return np.asarray(v, T)


def _norm(v):
    """Normalize: v / sqrt(x^2 + y^2 + z^2), the squares summed in order."""
    ln = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / ln[..., None]


def _len2(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def _safe_sqrt(x):
    return np.sqrt(np.where(x > 0, x, 0).astype(x.dtype))


def smooth_step(x, a, b, T):
    x, a, b = _t(T, x), T(a), T(b)
    if a == b:
        return np.where(x < a, T(0), T(1)).astype(T)
    t = np.clip((x - a) / (b - a), T(0), T(1))
    return (t * t * (T(3) - T(2) * t)).astype(T)


def light_position(rfl, T):
    """renderFromLight(Point3f(0, 0, 0)): the translation column (w = 1 for an affine matrix)."""
    m = _t(T, rfl)
    p = np.array([((m[r, 0] * T(0) + m[r, 1] * T(0)) + m[r, 2] * T(0)) + m[r, 3] for r in range(3)], T)
    w = ((m[3, 0] * T(0) + m[3, 1] * T(0)) + m[3, 2] * T(0)) + m[3, 3]
    return p if w == 1 else (p / w).astype(T)


def sample_li(kind, rfl, lfr, cos_start, cos_end, scale, I4, p, T=F32, mut=None):
    """(wi (n, 3), Li (n, 4), distance (n)) of Point/SpotLight::SampleLi at the points p (n, 3) with the
    intensity I4 (n, 4) at the path's wavelengths. A black Li is "no sample"."""
    if mut == "swapped":
        rfl, lfr = lfr, rfl
    pl = light_position(rfl, T)
    p, I4 = _t(T, p), _t(T, I4)
    d = (pl[None, :] - p).astype(T)
    wi = _norm(d)
    d2 = _len2(d)
    if kind == "spot":
        m = _t(T, lfr)[:3, :3]
        nw = -wi
        wl = np.stack([(m[r, 0] * nw[:, 0] + m[r, 1] * nw[:, 1]) + m[r, 2] * nw[:, 2] for r in range(3)], axis=1).astype(T)
        wl = _norm(wl)
        s = smooth_step(wl[:, 2], cos_end, cos_start, T)
        Li = ((s * T(scale))[:, None] * I4).astype(T)
    else:
        Li = (T(scale) * I4).astype(T)
    if mut != "no-r2":
        with np.errstate(invalid="ignore", divide="ignore"):
            Li = (Li / d2[:, None]).astype(T)
    return wi.astype(T), Li, np.sqrt(d2).astype(T)


# ---------------------------------------------------------------------------
# LightBounds, their union, and the build

class LB:
    def __init__(self, lo=None, hi=None, w=(0, 0, 0), phi=0.0, cos_o=0.0, cos_e=0.0, two=False):
        fmax = np.finfo(F32).max
        self.lo = np.full(3, fmax, F32) if lo is None else np.asarray(lo, F32)
        self.hi = np.full(3, -fmax, F32) if hi is None else np.asarray(hi, F32)
        self.w, self.phi = np.asarray(w, F32), F32(phi)
        self.cos_o, self.cos_e, self.two = F32(cos_o), F32(cos_e), bool(two)

    def centroid(self):
        return ((self.lo + self.hi) / F32(2)).astype(F32)


PI = F32(np.pi)


def point_bounds(rfl, scale, max_i):
    p = light_position(rfl, F32)
    phi = F32(F32(F32(F32(4) * PI) * F32(scale)) * F32(max_i))
    return LB(p, p, _norm(np.array([0, 0, 1], F32)), phi, np.cos(PI), np.cos(F32(PI / F32(2))), False)


def spot_bounds(rfl, scale, max_i, cos_start, cos_end):
    m = np.asarray(rfl, F32)
    p = light_position(m, F32)
    w = _norm(np.array([(m[r, 0] * F32(0) + m[r, 1] * F32(0)) + m[r, 2] * F32(1) for r in range(3)], F32))
    phi = F32(F32(F32(F32(scale) * F32(max_i)) * F32(4)) * PI)
    cos_e = F32(np.cos(F32(np.arccos(F32(cos_end)) - np.arccos(F32(cos_start)))))
    if cos_e == 1 and F32(cos_end) != F32(cos_start):
        cos_e = F32(0.999)
    return LB(p, p, _norm(w), phi, cos_start, cos_e, False)


def _safe_asin(x):
    return F32(np.arcsin(np.clip(F32(x), F32(-1), F32(1))))


def _safe_acos(x):
    return F32(np.arccos(np.clip(F32(x), F32(-1), F32(1))))


def _dot(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def _angle_between(a, b):
    if _dot(a, b) < 0:
        return F32(PI - F32(F32(2) * _safe_asin(F32(np.sqrt(_len2((a + b).astype(F32))) / F32(2)))))
    return F32(F32(2) * _safe_asin(F32(np.sqrt(_len2((b - a).astype(F32))) / F32(2))))


def _dop(a, b, c, d):
    """DifferenceOfProducts(a, b, c, d) = a b - c d through fma: exact products in float64."""
    cd = F32(F32(c) * F32(d))
    diff = F32(F64(a) * F64(b) - F64(cd))
    err = F32(-F64(c) * F64(d) + F64(cd))
    return F32(diff + err)


def _cone_union(wa, ca, wb, cb):
    """Union(DirectionCone, DirectionCone) -> (w, cosTheta); an empty cone has cosTheta = inf."""
    if ca == np.inf:
        return wb, cb
    if cb == np.inf:
        return wa, ca
    ta, tb = _safe_acos(ca), _safe_acos(cb)
    td = _angle_between(wa, wb)
    if min(F32(td + tb), PI) <= ta:
        return wa, ca
    if min(F32(td + ta), PI) <= tb:
        return wb, cb
    to = F32(F32(F32(ta + td) + tb) / F32(2))
    sphere = (np.array([0, 0, 1], F32), F32(-1))
    if to >= PI:
        return sphere
    tr = F32(to - ta)
    wr = np.array([_dop(wa[1], wb[2], wa[2], wb[1]), _dop(wa[2], wb[0], wa[0], wb[2]), _dop(wa[0], wb[1], wa[1], wb[0])],
                  F32)
    if _len2(wr) == 0:
        return sphere
    deg = F32(F32(F32(180) / PI) * tr)
    rad = F32(F32(PI / F32(180)) * deg)
    s, c = F32(np.sin(rad)), F32(np.cos(rad))
    a = _norm(wr).astype(F32)
    one = F32(1)
    m = np.array([
        [a[0] * a[0] + (one - a[0] * a[0]) * c, a[0] * a[1] * (one - c) - a[2] * s, a[0] * a[2] * (one - c) + a[1] * s],
        [a[0] * a[1] * (one - c) + a[2] * s, a[1] * a[1] + (one - a[1] * a[1]) * c, a[1] * a[2] * (one - c) - a[0] * s],
        [a[0] * a[2] * (one - c) - a[1] * s, a[1] * a[2] * (one - c) + a[0] * s, a[2] * a[2] + (one - a[2] * a[2]) * c]],
        F32)
    w = np.array([F32(F32(m[r, 0] * wa[0] + m[r, 1] * wa[1]) + m[r, 2] * wa[2]) for r in range(3)], F32)
    return _norm(w).astype(F32), F32(np.cos(to))


def lb_union(a, b):
    if a.phi == 0:
        return b
    if b.phi == 0:
        return a
    w, c = _cone_union(_norm(a.w).astype(F32), a.cos_o, _norm(b.w).astype(F32), b.cos_o)
    return LB(np.minimum(a.lo, b.lo), np.maximum(a.hi, b.hi), _norm(w).astype(F32), F32(a.phi + b.phi), c,
              min(a.cos_e, b.cos_e), a.two | b.two)


def evaluate_cost(b, lo, hi, dim):
    with np.errstate(all="ignore"):
        to, te = F32(np.arccos(b.cos_o)), F32(np.arccos(b.cos_e))
        tw = min(F32(to + te), PI)
        so = F32(np.sqrt(max(F32(0), F32(F32(1) - F32(b.cos_o * b.cos_o)))))
        m_omega = F32(F32(F32(F32(2) * PI) * F32(F32(1) - b.cos_o)) + F32(F32(PI / F32(2)) * F32(
            F32(F32(F32(F32(F32(2) * tw) * so) - F32(np.cos(F32(to - F32(F32(2) * tw))))) - F32(F32(F32(2) * to) * so))
            + b.cos_o)))
        d = (hi - lo).astype(F32)
        kr = F32(max(d[0], d[1], d[2]) / d[dim])
        e = (b.hi - b.lo).astype(F32)
        area = F32(F32(2) * F32(F32(F32(e[0] * e[1]) + F32(e[0] * e[2])) + F32(e[1] * e[2])))
        return F32(F32(F32(b.phi * m_omega) * kr) * area)


def _quantize_cos(c):
    return int(np.floor(F32(F32(32767) * F32(F32(F32(c) + F32(1)) / F32(2))))) & 0x7fff


def _quantize_bounds(c, lo, hi):
    if lo == hi:
        return F32(0)
    return F32(F32(65535) * np.clip(F32(F32(c - lo) / F32(hi - lo)), F32(0), F32(1)))


def _oct_encode(v):
    v = (v / F32(F32(abs(v[0]) + abs(v[1])) + abs(v[2]))).astype(F32)
    sign = lambda x: F32(np.copysign(F32(1), x))   # noqa: E731

    def enc(f):
        x = F32(np.clip(F32(F32(f + F32(1)) / F32(2)), F32(0), F32(1)) * F32(65535))
        return int(np.floor(F64(x) + 0.5))   # std::round of a non-negative value
    if v[2] >= 0:
        return enc(v[0]), enc(v[1])
    return enc(F32(F32(F32(1) - abs(v[1])) * sign(v[0]))), enc(F32(F32(F32(1) - abs(v[0])) * sign(v[1])))


def compact(lb, alo, ahi):
    wx, wy = _oct_encode(_norm(lb.w).astype(F32))
    qb = np.zeros((2, 3), np.int64)
    for c in range(3):
        qb[0, c] = int(np.floor(_quantize_bounds(lb.lo[c], alo[c], ahi[c])))
        qb[1, c] = int(np.ceil(_quantize_bounds(lb.hi[c], alo[c], ahi[c])))
    return dict(w=(wx, wy), phi=F32(lb.phi), qcos=(_quantize_cos(lb.cos_o), _quantize_cos(lb.cos_e)), two=lb.two, qb=qb)


def _partition(items, start, end, pred):
    """libstdc++'s std::partition for bidirectional iterators (bits/stl_algo.h __partition)."""
    first, last = start, end
    while True:
        while True:
            if first == last:
                return first
            if pred(items[first]):
                first += 1
            else:
                break
        last -= 1
        while True:
            if first == last:
                return first
            if not pred(items[last]):
                last -= 1
            else:
                break
        items[first], items[last] = items[last], items[first]
        first += 1


class Tree:
    """BVHLightSampler's members: nodes (dicts of compact() + link, leaf), all_lo / all_hi, infinite
    (list indices of the lights without bounds), n (the list's length)."""

    def __init__(self, bounds):
        """bounds: per light of the list None (an infinite light) or its LB."""
        fmax = np.finfo(F32).max
        self.n = len(bounds)
        self.nodes, self.infinite = [], []
        self.all_lo, self.all_hi = np.full(3, fmax, F32), np.full(3, -fmax, F32)
        lights = []
        for i, b in enumerate(bounds):
            if b is None:
                self.infinite.append(i)
            elif b.phi > 0:
                lights.append((i, b))
                self.all_lo, self.all_hi = np.minimum(self.all_lo, b.lo), np.maximum(self.all_hi, b.hi)
        if lights:
            self._build(lights, 0, len(lights))

    def _bucket(self, lb, clo, chi, dim):
        o = F32(lb.centroid()[dim] - clo[dim])
        if chi[dim] > clo[dim]:
            o = F32(o / F32(chi[dim] - clo[dim]))
        b = int(F32(F32(N_BUCKETS) * o))
        return N_BUCKETS - 1 if b == N_BUCKETS else b

    def _build(self, lights, start, end):
        if end - start == 1:
            node = compact(lights[start][1], self.all_lo, self.all_hi)
            node.update(link=lights[start][0], leaf=True, lb=lights[start][1])
            self.nodes.append(node)
            return len(self.nodes) - 1, lights[start][1]
        fmax = np.finfo(F32).max
        lo, hi = np.full(3, fmax, F32), np.full(3, -fmax, F32)
        clo, chi = lo.copy(), hi.copy()
        for _, lb in lights[start:end]:
            lo, hi = np.minimum(lo, lb.lo), np.maximum(hi, lb.hi)
            c = lb.centroid()
            clo, chi = np.minimum(clo, c), np.maximum(chi, c)
        min_cost, split_bucket, split_dim = F32(np.inf), -1, -1
        for dim in range(3):
            if chi[dim] == clo[dim]:
                continue
            buckets = [LB() for _ in range(N_BUCKETS)]
            for _, lb in lights[start:end]:
                k = self._bucket(lb, clo, chi, dim)
                buckets[k] = lb_union(buckets[k], lb)
            cost = []
            for i in range(N_BUCKETS - 1):
                b0, b1 = LB(), LB()
                for j in range(i + 1):
                    b0 = lb_union(b0, buckets[j])
                for j in range(i + 1, N_BUCKETS):
                    b1 = lb_union(b1, buckets[j])
                with np.errstate(all="ignore"):
                    cost.append(F32(evaluate_cost(b0, lo, hi, dim) + evaluate_cost(b1, lo, hi, dim)))
            for i in range(1, N_BUCKETS - 1):
                if cost[i] > 0 and cost[i] < min_cost:
                    min_cost, split_bucket, split_dim = cost[i], i, dim
        if split_dim == -1:
            mid = (start + end) // 2
        else:
            mid = _partition(lights, start, end, lambda l: self._bucket(l[1], clo, chi, split_dim) <= split_bucket)
            if mid == start or mid == end:
                mid = (start + end) // 2
        index = len(self.nodes)
        self.nodes.append(None)
        _, lb0 = self._build(lights, start, mid)
        second, lb1 = self._build(lights, mid, end)
        lb = lb_union(lb0, lb1)
        node = compact(lb, self.all_lo, self.all_hi)
        node.update(link=second, leaf=False, lb=lb)
        self.nodes[index] = node
        return index, lb


# ---------------------------------------------------------------------------
# CompactLightBounds::Importance and BVHLightSampler::Sample, vectorised over points

def _oct_decode(wx, wy, T):
    v = np.array([T(-1) + T(2) * (T(wx) / T(65535)), T(-1) + T(2) * (T(wy) / T(65535)), T(0)], T)
    v[2] = T(1) - (abs(v[0]) + abs(v[1]))
    if v[2] < 0:
        xo = v[0]
        v[0] = (T(1) - abs(v[1])) * T(np.copysign(1, xo))
        v[1] = (T(1) - abs(xo)) * T(np.copysign(1, v[1]))
    return _norm(v).astype(T)


def _lerp(x, a, b, T):
    return (T(1) - x) * a + x * b


def importance(node, all_lo, all_hi, p, T=F32, mut=None):
    """CompactLightBounds::Importance(p, n = 0, allb) of a node at the points p (n, 3).
    mut "unquantised": the node's exact bounds, cosines and direction (its LB) instead."""
    p = _t(T, p)
    alo, ahi = _t(T, all_lo), _t(T, all_hi)
    if mut == "unquantised":
        exact = node["lb"]
        lo, hi, w = _t(T, exact.lo), _t(T, exact.hi), _norm(_t(T, exact.w))
        cos_o, cos_e = T(exact.cos_o), T(exact.cos_e)
    else:
        qb = node["qb"]
        lo = np.array([_lerp(T(qb[0, c]) / T(65535), alo[c], ahi[c], T) for c in range(3)], T)
        hi = np.array([_lerp(T(qb[1, c]) / T(65535), alo[c], ahi[c], T) for c in range(3)], T)
        w = _oct_decode(node["w"][0], node["w"][1], T)
        cos_o = T(2) * (T(node["qcos"][0]) / T(32767)) - T(1)
        cos_e = T(2) * (T(node["qcos"][1]) / T(32767)) - T(1)
    phi = T(node["phi"])
    with np.errstate(all="ignore"):
        pc = ((lo + hi) / T(2)).astype(T)
        d2 = _len2((p - pc).astype(T))
        half = T(np.sqrt(_len2((hi - lo).astype(T))) / T(2))
        d2 = np.where(d2 < half, half, d2).astype(T)
        wi = _norm((p - pc).astype(T)).astype(T)
        cos_w = ((w[0] * wi[:, 0] + w[1] * wi[:, 1]) + w[2] * wi[:, 2]).astype(T)
        if node["two"]:
            cos_w = np.abs(cos_w)
        sin_w = _safe_sqrt((T(1) - cos_w * cos_w).astype(T))
        inside = bool(np.all(pc >= lo) and np.all(pc <= hi))
        radius = T(np.sqrt(_len2((pc - hi).astype(T)))) if inside else T(0)
        dist2 = _len2((p - pc).astype(T))
        sin2 = (radius * radius) / _len2((pc - p).astype(T))
        cos_b = np.where(dist2 < radius * radius, T(-1), _safe_sqrt((T(1) - sin2).astype(T))).astype(T)
        sin_b = _safe_sqrt((T(1) - cos_b * cos_b).astype(T))
        sin_o = T(np.sqrt(max(T(0), T(1) - cos_o * cos_o)))

        def cos_sub(sa, ca, sb, cb):
            return np.where(ca > cb, T(1), ca * cb + sa * sb).astype(T)

        def sin_sub(sa, ca, sb, cb):
            return np.where(ca > cb, T(0), sa * cb - ca * sb).astype(T)
        cos_x, sin_x = cos_sub(sin_w, cos_w, sin_o, cos_o), sin_sub(sin_w, cos_w, sin_o, cos_o)
        cos_p = cos_sub(sin_x, cos_x, sin_b, cos_b)
        imp = (phi * cos_p / d2).astype(T)
        imp = np.where(imp < 0, T(0), imp)
        return np.where(cos_p <= cos_e, T(0), imp).astype(T)


def bvh_sample(tree, p, u, T=F32, mut=None):
    """BVHLightSampler::Sample(ctx, u) at points p (n, 3) and draws u (n): (index in the light list
    or -1, pmf, margin). margin: how close the traversal came to a bin edge — the smallest
    |u' - edge| over the SampleDiscrete decisions taken, for the 1e-5 exclusion of the pick test.
    pInfinite and the infinite branch are ratios of light counts: they are evaluated in float32
    whatever T is (their bin edges are the sampler's own constants, not roundings of importances),
    so no draw is excluded on their account."""
    p, u = _t(T, p), _t(T, u).copy()
    n = len(u)
    idx, pmf, margin = np.full(n, -1, np.int64), np.zeros(n, T), np.full(n, np.inf)
    n_inf = len(tree.infinite)
    plus = 0 if (not tree.nodes or mut == "no-plus-one") else 1
    with np.errstate(all="ignore"):
        u32 = u.astype(F32)
        p_inf32 = F32(n_inf) / F32(n_inf + plus)
        p_inf = T(p_inf32)
        is_inf = u32 < p_inf32
        if n_inf:
            ui = (u32 / p_inf32).astype(F32)
            k = np.minimum((ui * F32(n_inf)).astype(np.int64), n_inf - 1)
            idx = np.where(is_inf, np.asarray(tree.infinite, np.int64)[k], idx)
            pmf = np.where(is_inf, T(p_inf32 / F32(n_inf)), pmf).astype(T)
        if not tree.nodes:
            return idx, pmf, margin
        active = ~is_inf
        uu = np.minimum(((u - p_inf) / (T(1) - p_inf)).astype(T), T(ONE_MINUS_EPS))
        pm = np.full(n, T(1) - p_inf, T)
        node_i = np.zeros(n, np.int64)
        while active.any():
            for ni in np.unique(node_i[active]):
                sel = active & (node_i == ni)
                node = tree.nodes[ni]
                if node["leaf"]:
                    ok = np.ones(sel.sum(), bool)
                    if ni == 0:
                        ok = importance(node, tree.all_lo, tree.all_hi, p[sel], T, mut) > 0
                    idx[sel] = np.where(ok, node["link"], -1)
                    pmf[sel] = np.where(ok, pm[sel], T(0))
                    active[sel] = False
                    continue
                c0, c1 = ni + 1, node["link"]
                w0 = importance(tree.nodes[c0], tree.all_lo, tree.all_hi, p[sel], T, mut)
                w1 = importance(tree.nodes[c1], tree.all_lo, tree.all_hi, p[sel], T, mut)
                none = (w0 == 0) & (w1 == 0)
                # SampleDiscrete over {w0, w1}
                total = ((T(0) + w0) + w1).astype(T)
                up = (uu[sel] * total).astype(T)
                up = np.where(up == total, np.nextafter(up, T(-np.inf)), up).astype(T)
                second = (T(0) + w0) <= up
                chosen = np.where(second, w1, w0)
                base = np.where(second, (T(0) + w0).astype(T), T(0))
                npmf = (chosen / total).astype(T)
                unew = np.minimum(((up - base) / chosen).astype(T), T(ONE_MINUS_EPS))
                m = np.abs(uu[sel].astype(F64) - w0.astype(F64) / total.astype(F64))
                margin[sel] = np.where(none, margin[sel], np.minimum(margin[sel], m))
                s_idx = np.flatnonzero(sel)
                dead = s_idx[none]
                idx[dead], pmf[dead], active[dead] = -1, 0, False
                live = s_idx[~none]
                uu[live] = unew[~none]
                pm[live] = (pm[live] * npmf[~none]).astype(T)
                node_i[live] = np.where(second[~none], c1, c0)
    return idx, pmf, margin


def pmf_infinite(tree, T=F32, mut=None):
    """BVHLightSampler::PMF of an infinite light."""
    plus = 0 if (not tree.nodes or mut == "no-plus-one") else 1
    with np.errstate(divide="ignore"):      # no light at all: 1 / 0, as the reference's
        return T(1) / T(len(tree.infinite) + plus)


# ---------------------------------------------------------------------------
# Create

def point_scale(scale, photometric, power=None):
    sc = F32(F32(scale) / F32(photometric))
    if power is not None and power > 0:
        sc = F32(sc * F32(F32(power) / F32(F32(4) * PI)))
    return sc


def spot_cosines(coneangle, conedelta):
    rad = lambda deg: F32(F32(PI / F32(180)) * F32(deg))   # noqa: E731
    return F32(np.cos(rad(F32(F32(coneangle) - F32(conedelta))))), F32(np.cos(rad(coneangle)))


def spot_scale(scale, photometric, coneangle, conedelta, power=None):
    sc = F32(F32(scale) / F32(photometric))
    if power is not None and power > 0:
        cs, ce = spot_cosines(coneangle, conedelta)
        k_e = F32(F32(F32(2) * PI) * F32(F32(F32(1) - cs) + F32(F32(cs - ce) / F32(2))))
        sc = F32(sc * F32(F32(power) / k_e))
    return sc
