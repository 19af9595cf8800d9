// Host-side sanitizer run of the uniform lighting graph (avr_graph_uniform.h, the host code of
// avr_graph_uniform_*). Built by tests/test_graph_uniform.py with g++
// -fsanitize=address,undefined -fno-sanitize-recover=all and run as an executable: create and
// its argument errors, the conversion from points (first and mean), lookups (random points,
// exact half-way points, NaN, far outside the range) and the first-lit-voxel search
// (orthographic and perspective rays, axis-parallel, zero and non-finite directions, origins
// inside the bounds). Any out-of-bounds access, leak or undefined behaviour aborts.
#include "../acceleratedvolrenderer_amd/csrc/avr_graph_uniform.h"

#include <cstdio>
#include <limits>
#include <random>
#include <vector>

using avr::graph::Uniform;

static int fail(const char *what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

int main() {
    std::mt19937 gen(7);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

    // create: lit voxels of a ball on the lattice 0..12 at spacing 1/12, a third dropped, some dark
    const float s = 1.f / 12.f;
    std::vector<int> coors;
    std::vector<float> light;
    for (int x = 0; x <= 12; ++x)
        for (int y = 0; y <= 12; ++y)
            for (int z = 0; z <= 12; ++z) {
                const float dx = x * s - 0.5f, dy = y * s - 0.5f, dz = z * s - 0.5f;
                if (dx * dx + dy * dy + dz * dz > 0.42f * 0.42f || U(gen) < 1.f / 3.f) continue;
                coors.insert(coors.end(), {x, y, z});
                light.push_back(U(gen) < 0.1f ? 0.f : 0.05f + U(gen));
            }
    const long long m = (long long)light.size();
    Uniform ball;
    if (!ball.Create(m, coors.data(), light.data(), s).empty()) return fail("create");
    if (ball.NumVertices() != (size_t)m || ball.Capacity() < 2 * (size_t)m) return fail("size");

    // argument errors leave nothing behind
    {
        Uniform bad;
        if (bad.Create(m, coors.data(), light.data(), 0.f).empty()) return fail("spacing 0");
        if (bad.Create(m, coors.data(), light.data(), nan).empty()) return fail("spacing NaN");
        if (bad.Create(0, coors.data(), light.data(), s).empty()) return fail("m 0");
        std::vector<int> c2(coors.begin(), coors.begin() + 6);
        std::vector<float> l2(light.begin(), light.begin() + 2);
        c2[3] = 1 << 20;
        if (bad.Create(2, c2.data(), l2.data(), s).find("vertex 1") == std::string::npos) return fail("coordinate range");
        c2[3] = c2[0], c2[4] = c2[1], c2[5] = c2[2];
        if (bad.Create(2, c2.data(), l2.data(), s).find("vertex 1") == std::string::npos) return fail("repeated");
        c2[3] = c2[0] + 1;
        l2[0] = nan;
        if (bad.Create(2, c2.data(), l2.data(), s).find("vertex 0") == std::string::npos) return fail("NaN light");
        l2[0] = 1.f;
        c2[0] = -(1 << 20) + 1, c2[3] = (1 << 20) - 1;   // the extreme valid coordinates
        if (!bad.Create(2, c2.data(), l2.data(), s).empty()) return fail("extreme coordinates");
        const float far[6] = {c2[0] * s, c2[1] * s, c2[2] * s, c2[3] * s, c2[4] * s, c2[5] * s};
        int id[2];
        bad.Lookup(2, far, id, nullptr);
        if (id[0] != 0 || id[1] != 1) return fail("extreme lookup");
        const float o[3] = {far[0] - 1.f, far[1], far[2]}, d[3] = {1.f, 0.f, 0.f};
        float h0, h1;
        bad.Trace(1, o, d, id, &h0, &h1);   // a walk across the whole coordinate range
        if (id[0] != 0) return fail("extreme trace");
    }

    // from_points: 4000 random vertices at spacing 0.08, first and mean
    const int n = 4000;
    std::vector<float> pts(3 * n), pl(n);
    for (auto &v : pts) v = U(gen);
    for (auto &v : pl) v = U(gen);
    std::vector<int> vertexOf(n);
    for (int reduce = 0; reduce < 2; ++reduce) {
        Uniform u;
        if (!u.FromPoints(n, pts.data(), pl.data(), 0.08f, reduce, vertexOf.data()).empty()) return fail("from_points");
        std::vector<int> id(n);
        std::vector<float> l(n);
        u.Lookup(n, pts.data(), id.data(), l.data());
        for (int i = 0; i < n; ++i)
            if (id[i] != vertexOf[i] || l[i] != u.Light()[id[i]]) return fail("from_points lookup");
        pts[5] = nan;
        if (u.FromPoints(n, pts.data(), pl.data(), 0.08f, reduce, nullptr).find("vertex 1") == std::string::npos)
            return fail("NaN point");
        pts[5] = 0.5f;
        if (u.FromPoints(n, pts.data(), pl.data(), 0.08f, 2, nullptr).empty()) return fail("reduce");
    }

    // lookups: random, half-way, NaN, beyond +-2^20 spacing
    std::vector<float> q;
    for (int i = 0; i < 4000 * 3; ++i) q.push_back(-0.3f + 1.6f * U(gen));
    for (int k = -8; k <= 20; ++k)
        for (int a = 0; a < 3; ++a) q.push_back(((float)k + 0.5f) * s);
    for (float v : {nan, inf, -inf, 1e30f, -1e30f, (float)(1 << 20) * s, -(float)(1 << 20) * s})
        q.insert(q.end(), {v, 0.5f, 0.5f});
    std::vector<int> qid(q.size() / 3);
    std::vector<float> ql(q.size() / 3);
    ball.Lookup((long long)qid.size(), q.data(), qid.data(), ql.data());
    for (size_t i = qid.size() - 7; i < qid.size(); ++i)
        if (qid[i] != -1 || ql[i] != 0.f) return fail("invalid coordinate");

    // trace: orthographic rays along +z, perspective rays, and degenerate ones
    std::vector<float> o, d;
    for (int i = 0; i < 4096; ++i) {
        o.insert(o.end(), {U(gen), U(gen), -1.f});
        d.insert(d.end(), {0.f, 0.f, 1.f});
    }
    for (int i = 0; i < 4096; ++i) {
        float v[3] = {-0.1f + 1.2f * U(gen) - 0.5f, -0.1f + 1.2f * U(gen) - 0.5f, 2.f};
        const float len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        o.insert(o.end(), {0.5f, 0.5f, -1.5f});
        d.insert(d.end(), {v[0] / len, v[1] / len, v[2] / len});
    }
    const float odd[][6] = {{0.5f, 0.5f, 0.5f, 0.f, 0.f, 0.f},  {0.5f, 0.5f, 0.5f, -1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f, nan, 0.f, 1.f},
                            {nan, 0.5f, 0.5f, 0.f, 0.f, 1.f},   {inf, 0.5f, 0.5f, -1.f, 0.f, 0.f},  {0.5f, 0.5f, -1.f, 0.f, 0.f, inf},
                            {0.5f, 0.5f, 5.f, 0.f, 0.f, 1.f},   {3.f, 3.f, 3.f, -1.f, -1.f, -1.f},  {0.5f, 0.5f, -1e30f, 0.f, 0.f, 1.f},
                            {0.5f, 0.5f, -1.f, 1e-30f, 0.f, 1.f}};
    for (const auto &r : odd) {
        o.insert(o.end(), r, r + 3);
        d.insert(d.end(), r + 3, r + 6);
    }
    const long long nr = (long long)o.size() / 3;
    std::vector<int> tid(nr);
    std::vector<float> h0(nr), h1(nr);
    ball.Trace(nr, o.data(), d.data(), tid.data(), h0.data(), h1.data());
    long long hits = 0;
    for (long long i = 0; i < nr; ++i) {
        if (tid[i] < -1 || tid[i] >= m) return fail("trace id");
        if (tid[i] >= 0) {
            ++hits;
            if (ball.Light()[tid[i]] == 0.f || !(h0[i] <= h1[i])) return fail("trace hit");
        }
    }
    if (hits < 2000) return fail("too few rays hit");
    std::printf("sanitize ok: %lld vertices, %lld of %lld rays hit\n", m, hits, nr);
    return 0;
}
