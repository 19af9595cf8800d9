// Host-side sanitizer run of the voxel boundary's floods (avr_graph_voxels.h, the host code of
// avr_graph_voxels_*) and of the conversion from points they start from (Uniform::FromPoints).
// Built by tests/test_graph_voxels.py with g++ -fsanitize=address,undefined
// -fno-sanitize-recover=all and run as an executable: create and its argument errors, the
// single layer and the fill (lowest start, every start, an explicit start, bad starts) on a
// hollow shell, an L-shaped solid and a shell with a one-voxel hole, and a point cloud through
// FromPoints into the floods. Any out-of-bounds access, leak or undefined behaviour aborts.
#include "../acceleratedvolrenderer_amd/csrc/avr_graph_voxels.h"

#include <cstdio>
#include <limits>
#include <random>
#include <vector>

using namespace avr::graph;

static int fail(const char *what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

static std::vector<int> shell(bool hole) {
    std::vector<int> c;
    for (int x = 0; x <= 11; ++x)
        for (int y = 0; y <= 11; ++y)
            for (int z = 0; z <= 11; ++z) {
                const float dx = x - 5.5f, dy = y - 5.5f, dz = z - 5.5f, r = std::sqrt(dx * dx + dy * dy + dz * dz);
                if (r < 3.6f || r >= 4.7f || (hole && x == 10 && y == 5 && z == 5)) continue;
                c.insert(c.end(), {x, y, z});
            }
    return c;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {11.f, 11.f, 11.f};

    // the closed shell: the inside is filled, the outside is not
    const std::vector<int> sc = shell(false);
    const long long m = (long long)sc.size() / 3;
    Voxels v;
    if (!v.Create(lo, hi, 1.f, m, sc.data()).empty()) return fail("create shell");
    if (v.Dims().cells != 14 * 14 * 14) return fail("shell lattice");
    if (v.Fill(-1, nullptr).empty()) return fail("fill before the single layer must be refused");
    int levels = 0;
    v.SingleLayer(&levels);
    if (levels < 14 || v.Count(kVoxOutside) + m >= 14 * 14 * 14) return fail("shell single layer");
    const long long inside = 14 * 14 * 14 - v.Count(kVoxOutside) - m;
    if (!v.Fill(-1, &levels).empty() || v.Count(kVoxFilled) != m + inside) return fail("shell fill");
    if (!v.Fill(-2, &levels).empty() || v.Count(kVoxFilled) != m + inside) return fail("shell fill from all");
    if (v.Fill((int)m, nullptr).empty() || v.Fill(-3, nullptr).empty() || v.Fill(0x7fffffff, nullptr).empty())
        return fail("bad start accepted");
    for (long long s = 0; s < m; ++s) {   // every vertex as a start: refused or the same fill
        if (v.Fill((int)s, nullptr).empty() && v.Count(kVoxFilled) != m + inside) return fail("shell fill from a vertex");
    }

    // the hole lets the first flood in: nothing but vertices is left to fill
    const std::vector<int> hc = shell(true);
    Voxels h;
    if (!h.Create(lo, hi, 1.f, m - 1, hc.data()).empty()) return fail("create hole");
    h.SingleLayer(nullptr);
    if (h.Count(kVoxOutside) + (m - 1) != 14 * 14 * 14) return fail("hole leak");
    if (!h.Fill(-1, nullptr).empty() || h.Count(kVoxFilled) > m - 1) return fail("hole fill");
    if (!h.Fill(-2, nullptr).empty() || h.Count(kVoxFilled) != m - 1) return fail("hole fill from all");

    // the L-shaped solid at spacing 1/4 on a non-cubic lattice
    std::vector<int> lc;
    for (int x = 1; x <= 8; ++x)
        for (int y = 1; y <= 8; ++y)
            for (int z = 1; z <= 4; ++z)
                if (!(x >= 5 && y >= 5)) lc.insert(lc.end(), {x, y, z});
    const float lhi[3] = {9 * 0.25f, 9 * 0.25f, 5 * 0.25f};
    Voxels l;
    if (!l.Create(lo, lhi, 0.25f, (long long)lc.size() / 3, lc.data()).empty()) return fail("create L");
    if (l.Dims().n[0] != 12 || l.Dims().n[2] != 8) return fail("L lattice");
    l.SingleLayer(nullptr);
    if (l.Count(kVoxSingle) >= (long long)lc.size() / 3 || l.Count(kVoxSingle) == 0) return fail("L single layer");
    if (!l.Fill(-2, nullptr).empty() || l.Count(kVoxFilled) != (long long)lc.size() / 3) return fail("L fill");

    // argument errors
    Voxels e;
    const int out[6] = {1, 1, 1, 13, 1, 1}, twice[6] = {1, 1, 1, 1, 1, 1};
    const float big[3] = {3000.f, 3000.f, 3000.f};
    if (e.Create(lo, hi, 0.f, 1, out).empty() || e.Create(lo, hi, nan, 1, out).empty() || e.Create(lo, hi, -1.f, 1, out).empty())
        return fail("bad spacing accepted");
    if (e.Create(lo, hi, 1.f, 0, out).empty() || e.Create(lo, hi, 1.f, 1, nullptr).empty() || e.Create(nullptr, hi, 1.f, 1, out).empty())
        return fail("empty input accepted");
    if (e.Create(lo, hi, 1.f, 2, out).empty() || e.Create(lo, hi, 1.f, 2, twice).empty()) return fail("bad vertex accepted");
    if (e.Create(lo, big, 1.f, 1, out).empty()) return fail("cell cap");
    if (e.Create(lo, big, 1e-9f, 1, out).empty()) return fail("bounds beyond the coordinate range");

    // a point cloud on a sphere through FromPoints into the floods
    std::mt19937 gen(3);
    std::normal_distribution<float> N(0.f, 1.f);
    std::vector<float> pts, light;
    for (int i = 0; i < 20000; ++i) {
        const float x = N(gen), y = N(gen), z = N(gen), r = std::sqrt(x * x + y * y + z * z);
        if (!(r > 1e-3f)) continue;
        pts.insert(pts.end(), {0.5f + 0.4f * x / r, 0.5f + 0.4f * y / r, 0.5f + 0.4f * z / r});
        light.push_back(0.f);
    }
    Uniform u;
    std::vector<int> vertex_of(light.size());
    if (!u.FromPoints((long long)light.size(), pts.data(), light.data(), 1.f / 16.f, 0, vertex_of.data()).empty())
        return fail("from points");
    const float ulo[3] = {0.f, 0.f, 0.f}, uhi[3] = {1.f, 1.f, 1.f};
    Voxels c;
    if (!c.Create(ulo, uhi, u.Spacing(), (long long)u.NumVertices(), u.Coors()).empty()) return fail("create cloud");
    c.SingleLayer(nullptr);
    if (!c.Fill(-1, nullptr).empty()) return fail("cloud fill");
    if (c.Count(kVoxFilled) <= (long long)u.NumVertices() || c.Count(kVoxCast) == 0) return fail("cloud counts");
    pts[4] = nan;
    if (u.FromPoints((long long)light.size(), pts.data(), light.data(), 1.f / 16.f, 0, nullptr).empty())
        return fail("NaN point accepted");

    std::printf("sanitize ok: shell %lld vertices, %lld inside; cloud %zu vertices, %lld filled\n", m, inside, u.NumVertices(),
                c.Count(kVoxFilled));
    return 0;
}
