// avr_graph_voxels.h — the voxel boundary's two floods: VoxelBoundary::ToSingleLayerAndSaveCast
// (graph/voxels/voxel_boundary.cpp:122-181) and FillInside (:183-225). One set of cell rules,
// compiled for the host (Voxels::SingleLayer / Fill: plain breadth-first loops) and for the
// device (k_graph_voxels_level: one launch per level over a frontier list): the semantics below
// are the contract of both, and the state bytes they leave are the same.
//
// State: one byte per cell of the dense lattice over FitBounds (util.h:313-317): lo =
// FitToGraph(pmin) - 1, hi = FitToGraph(pmax) + 1 per axis, inclusive, pmin / pmax the bounds of
// the medium's primitive; cell = (cx - lo.x) + nx ((cy - lo.y) + ny (cz - lo.z)), x fastest.
//   1  boundary vertex (given)            8  single-layer vertex
//   2  outside: visited by the first flood   16 filled
//   4  cast
// At most 2^31 - 1 cells; a vertex outside the bounds is refused (the reference's sets would
// hold it, but no flood could reach it).
//
// Single layer (voxel_visit_outside): the flood starts at lo, which is visited whatever it holds,
// and spreads over 6-neighbours inside the bounds that are not vertices. A visited cell with a
// vertex neighbour is cast; a vertex with a visited neighbour is single-layer. The reference's
// three sets (previous, current, next level) are a level-synchronous breadth-first search in
// which each cell is visited once: its numVisited is the number of cells with bit 2.
//
// Fill (voxel_visit_fill): the seeds are filled, and the flood spreads over 6-neighbours inside
// the bounds that are not cast. Every result is a set, so neither flood depends on the order
// in which a level's cells are taken.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "avr_graph_uniform.h"

namespace avr {
namespace graph {

constexpr unsigned kVoxVertex = 1, kVoxOutside = 2, kVoxCast = 4, kVoxSingle = 8, kVoxFilled = 16;
constexpr long long kVoxMaxCells = 0x7fffffffll;

struct VoxelDims {
    int lo[3];
    int n[3];
    int cells;
};

// The 6-neighbour k of `cell` (k / 2 the axis, even k: -1, odd: +1, GetNeighbours :106-120), or
// -1 outside the bounds; (x, y, z) are the cell's own lattice offsets
AVR_HD int voxel_neighbour(const VoxelDims &d, int cell, int x, int y, int z, int k) {
    const int s = (k & 1) ? 1 : -1;
    if (k < 2) return (unsigned)(x + s) < (unsigned)d.n[0] ? cell + s : -1;
    if (k < 4) return (unsigned)(y + s) < (unsigned)d.n[1] ? cell + s * d.n[0] : -1;
    return (unsigned)(z + s) < (unsigned)d.n[2] ? cell + s * d.n[0] * d.n[1] : -1;
}

// One visited cell of the first flood. St: bits(cell) reads a cell's byte, set(cell, bit) ors a
// bit in and returns whether it was clear before (exactly one caller sees true). push(nb) takes
// the neighbours that join the next level.
template <typename St, typename Push>
AVR_HD void voxel_visit_outside(const VoxelDims &d, St &st, int cell, Push push) {
    const int x = cell % d.n[0], yz = cell / d.n[0], y = yz % d.n[1], z = yz / d.n[1];
    bool cast = false;
    for (int k = 0; k < 6; ++k) {
        const int nb = voxel_neighbour(d, cell, x, y, z, k);
        bool fresh = false;
        if (nb >= 0) {
            const unsigned b = st.bits(nb);
            if (b & kVoxVertex) {
                cast = true;
                if (!(b & kVoxSingle)) (void)st.set(nb, kVoxSingle);
            } else if (!(b & kVoxOutside)) {
                fresh = st.set(nb, kVoxOutside);
            }
        }
        push(nb, fresh);
    }
    if (cast) (void)st.set(cell, kVoxCast);
}

// One visited cell of the fill
template <typename St, typename Push>
AVR_HD void voxel_visit_fill(const VoxelDims &d, St &st, int cell, Push push) {
    const int x = cell % d.n[0], yz = cell / d.n[0], y = yz % d.n[1], z = yz / d.n[1];
    for (int k = 0; k < 6; ++k) {
        const int nb = voxel_neighbour(d, cell, x, y, z, k);
        bool fresh = false;
        if (nb >= 0) {
            const unsigned b = st.bits(nb);
            if (!(b & (kVoxCast | kVoxFilled))) fresh = st.set(nb, kVoxFilled);
        }
        push(nb, fresh);
    }
}

struct VoxelStateHost {
    uint8_t *s;
    unsigned bits(int cell) const { return s[cell]; }
    bool set(int cell, unsigned bit) {
        const bool clear = !(s[cell] & bit);
        s[cell] = (uint8_t)(s[cell] | bit);
        return clear;
    }
};

// The host state and floods (avr_graph_voxels_*). Create returns a message on a bad argument,
// else an empty string.
class Voxels {
  public:
    std::string Create(const float pmin[3], const float pmax[3], float spacing, long long m, const int *coors) {
        if (!(spacing > 0) || !std::isfinite(spacing)) return "graph voxels: spacing must be positive and finite";
        if (!pmin || !pmax) return "graph voxels: null bounds";
        if (m < 1 || m > 0x3fffffff || !coors) return "graph voxels: at least one vertex required";
        int lo[3], hi[3];
        if (!uniform_coors(pmin[0], pmin[1], pmin[2], spacing, lo) || !uniform_coors(pmax[0], pmax[1], pmax[2], spacing, hi))
            return "graph voxels: bounds outside +-2^20 voxels";
        long long cells = 1;
        for (int a = 0; a < 3; ++a) {
            lo[a] -= 1;
            hi[a] += 1;
            if (hi[a] < lo[a]) return "graph voxels: empty bounds";
            d_.lo[a] = lo[a];
            d_.n[a] = hi[a] - lo[a] + 1;
            cells *= d_.n[a];
            if (cells > kVoxMaxCells) return "graph voxels: more than 2^31 - 1 cells";
        }
        d_.cells = (int)cells;
        spacing_ = spacing;
        // padded to whole 32-bit words: the device ors bits into the word that holds a byte
        state_.assign(((size_t)cells + 3) & ~(size_t)3, 0);
        cell_of_.resize((size_t)m);
        for (long long v = 0; v < m; ++v) {
            const int *c = coors + 3 * v;
            for (int a = 0; a < 3; ++a)
                if (c[a] < lo[a] || c[a] > hi[a]) return "graph voxels: vertex " + std::to_string(v) + ": outside the bounds";
            const int cell = (c[0] - lo[0]) + d_.n[0] * ((c[1] - lo[1]) + d_.n[1] * (c[2] - lo[2]));
            if (state_[(size_t)cell] & kVoxVertex) return "graph voxels: vertex " + std::to_string(v) + ": repeated coordinate";
            state_[(size_t)cell] = kVoxVertex;
            cell_of_[(size_t)v] = cell;
        }
        single_done_ = false;
        return "";
    }

    // The first flood's start: bits 2 to 16 cleared, lo visited
    void BeginSingleLayer(std::vector<int> *frontier) {
        for (auto &b : state_) b &= (uint8_t)kVoxVertex;
        state_[0] |= (uint8_t)kVoxOutside;
        frontier->assign(1, 0);
    }
    void SingleLayer(int *levels) {
        std::vector<int> cur, next;
        BeginSingleLayer(&cur);
        VoxelStateHost st{state_.data()};
        int lv = 0;
        while (!cur.empty()) {
            ++lv;
            next.clear();
            for (int cell : cur)
                voxel_visit_outside(d_, st, cell, [&](int nb, bool fresh) {
                    if (fresh) next.push_back(nb);
                });
            cur.swap(next);
        }
        single_done_ = true;
        if (levels) *levels = lv;
    }

    // The fill's start. start >= 0: that vertex; -1: the lowest single-layer vertex; -2: every
    // single-layer vertex. A message when the start is no single-layer vertex.
    std::string BeginFill(int start, std::vector<int> *frontier) {
        if (!single_done_) return "graph voxels: single layer has not run";
        frontier->clear();
        if (start >= 0) {
            if ((size_t)start >= cell_of_.size() || !(state_[(size_t)cell_of_[(size_t)start]] & kVoxSingle))
                return "graph voxels: start " + std::to_string(start) + " is no single-layer vertex";
            frontier->push_back(cell_of_[(size_t)start]);
        } else if (start == -1 || start == -2) {
            for (size_t v = 0; v < cell_of_.size(); ++v)
                if (state_[(size_t)cell_of_[v]] & kVoxSingle) {
                    frontier->push_back(cell_of_[v]);
                    if (start == -1) break;
                }
            if (frontier->empty()) return "graph voxels: no single-layer vertex to start from";
        } else {
            return "graph voxels: start is a vertex id, -1 (lowest) or -2 (all)";
        }
        for (auto &b : state_) b &= (uint8_t)~kVoxFilled;
        for (int cell : *frontier) state_[(size_t)cell] |= (uint8_t)kVoxFilled;
        return "";
    }
    std::string Fill(int start, int *levels) {
        std::vector<int> cur, next;
        const std::string msg = BeginFill(start, &cur);
        if (!msg.empty()) return msg;
        VoxelStateHost st{state_.data()};
        int lv = 0;
        while (!cur.empty()) {
            ++lv;
            next.clear();
            for (int cell : cur)
                voxel_visit_fill(d_, st, cell, [&](int nb, bool fresh) {
                    if (fresh) next.push_back(nb);
                });
            cur.swap(next);
        }
        if (levels) *levels = lv;
        return "";
    }

    long long Count(unsigned bit) const {
        long long n = 0;
        for (int i = 0; i < d_.cells; ++i) n += (state_[(size_t)i] & bit) ? 1 : 0;
        return n;
    }
    const VoxelDims &Dims() const { return d_; }
    uint8_t *State() { return state_.data(); }
    const uint8_t *State() const { return state_.data(); }
    size_t StateBytes() const { return state_.size(); }
    bool SingleDone() const { return single_done_; }
    void SetSingleDone() { single_done_ = true; }
    float Spacing() const { return spacing_; }

  private:
    VoxelDims d_{};
    float spacing_ = 1;
    std::vector<uint8_t> state_;
    std::vector<int> cell_of_;
    bool single_done_ = false;
};

}  // namespace graph
}  // namespace avr
