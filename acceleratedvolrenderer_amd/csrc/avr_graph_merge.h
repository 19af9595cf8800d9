// avr_graph_merge.h — the vertex merge of FreeGraphBuilder::TracePath (free_graph_builder.cpp:
// 71-93, Builder::AddWalk in avr_graph_host.h) as data-parallel rounds: which vertex every
// scatter point of a batch of walks belongs to. One step routine, compiled for the host
// (avr_graph_merge_assign) and for the device (k_graph_merge_round): the semantics below are the
// contract of both, and their answer is Builder::AddWalk's.
//
// Entities are numbered by sequence: the graph's existing vertices first (seq = id, V0 of
// them), then the call's scatter points in walk order, then point order. Vertex ids grow with
// seq. AddWalk gives point i (a) the nearest vertex existing at its turn with float
// d2 = dx*dx + dy*dy + dz*dz < r2 (ties: lowest id), else (b) its path's previous vertex when
// that one's d2 <= r2 (d2 == r2 then), else (c) a new vertex at its own position. Positions
// never move, so a point's answer depends only on which lower-seq entities within the radius
// are vertices, and on its walk predecessor's vertex.
//
// State per point, one int that only moves forward: kMergeUndecided -> kMergePending (a lower
// vertex lies within the radius: the point will merge and is no candidate for anyone) -> the
// seq of its vertex (>= 0: final; its own seq: the point is a new vertex). merge_step(i):
//   - scans the lower-seq entities with d2 < r2: existing vertices and new points are
//     candidates (minimum of (d2, seq)), pending and merged points are skipped, undecided
//     ones are noted;
//   - a candidate and no undecided point before it in (d2, seq) order (one behind it cannot
//     become the target): final, the best candidate; a candidate otherwise: pending;
//   - no candidate and nothing undecided, and the walk predecessor final (or none): the
//     previous vertex when its d2 <= r2, else new.
// A state once written is the sequential answer, so a step may read states that other lanes
// write during the same sweep (the device: relaxed atomics at agent scope) or the states of
// the round before (the host: synchronous rounds); fresher states only save rounds. The
// unfinalised point of lowest seq can always be finalised, so every round finalises at least
// one point and the fixed point is the sequential result.
//
// Search: a cell grid over all entities of the call (MergeGrid), sized as the vertex index's
// (cell edge = vertex radius, doubled until at most kIndexCellBudget cells), entities
// counting-sorted by cell (ascending seq within a cell), one 16-B record {x, y, z, seq} each.
// A query's cells follow index_cell_range: double arithmetic on the radius widened by 1e-6
// relative, so cell rounding never hides an entity whose float d2 qualifies. (AddWalk's own
// hash grid floors float x / r per axis and visits 27 cells; a pair whose two quotients round
// across a cell border in opposite directions while d2 < r2 holds by an ulp could escape it.
// The rule here is the one AddWalk documents, d2 < r2 over every vertex.)
#pragma once

#include "avr_graph_index.h"

namespace avr {
namespace graph {

constexpr int kMergeUndecided = -1, kMergePending = -2;

struct alignas(16) MergeRec { float x, y, z; int seq; };

// What a step reads: the host grid's arrays, or their device copies
struct MergeView {
    const MergeRec *rec;      // every entity, sorted by cell
    const MergeRec *ent;      // every entity by seq
    const int *cell_start;    // dim[0] * dim[1] * dim[2] + 1 offsets into rec
    const int *prev;          // per point: seq of the walk's previous entity (a start vertex or a point), -1 none
    double bmin[3], inv_cell, reach;
    int dim[3];
    int v0, n;                // existing vertices, points
    float r2;                 // Sqr(vertexRadius)
};

// What a scan of the entities around a point found: the smallest keys (d2, seq) among the
// vertices in range (best, -1: none) and among the undecided points (open, -1: none)
struct MergeScan {
    int best, open;
    float bestD, openD;
};

AVR_HD void merge_scan_take(int *id, float *d, int seq, float d2) {
    if (*id < 0 || d2 < *d || (d2 == *d && seq < *id)) {
        *id = seq;
        *d = d2;
    }
}

// Two partial scans of one point into one
AVR_HD void merge_scan_join(MergeScan *a, const MergeScan &b) {
    if (b.best >= 0) merge_scan_take(&a->best, &a->bestD, b.best, b.bestD);
    if (b.open >= 0) merge_scan_take(&a->open, &a->openD, b.open, b.openD);
}

// The lower-seq entities with d2 < r2 around point seq at q over the state accessor st (int
// load(int point), void store(int point, int value)); part `lane` of `lanes`: every lanes-th
// record of each run of cells (the whole scan: 0 of 1; a wave sharing one point: its lanes,
// joined afterwards)
template <typename St>
AVR_HD MergeScan merge_scan(const MergeView &mv, int seq, const MergeRec &q, St &st, int lane, int lanes) {
    MergeScan r{-1, -1, 0.f, 0.f};
    int lo[3], hi[3];
    if (!index_cell_range((double)q.x, mv.reach, mv.bmin[0], mv.inv_cell, mv.dim[0], &lo[0], &hi[0]) ||
        !index_cell_range((double)q.y, mv.reach, mv.bmin[1], mv.inv_cell, mv.dim[1], &lo[1], &hi[1]) ||
        !index_cell_range((double)q.z, mv.reach, mv.bmin[2], mv.inv_cell, mv.dim[2], &lo[2], &hi[2]))
        return r;
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y) {
            // the cells of one x run are contiguous in the sorted records
            const long long row = ((long long)z * mv.dim[1] + y) * mv.dim[0];
            const int s0 = mv.cell_start[row + lo[0]], s1 = mv.cell_start[row + hi[0] + 1];
            for (int s = s0 + lane; s < s1; s += lanes) {
                const MergeRec v = mv.rec[s];
                if (v.seq >= seq) continue;
                const float dx = v.x - q.x, dy = v.y - q.y, dz = v.z - q.z;
                const float d2 = dx * dx + dy * dy + dz * dz;
                if (!(d2 < mv.r2)) continue;
                if (v.seq >= mv.v0) {
                    const int t = st.load(v.seq - mv.v0);
                    if (t == kMergeUndecided) {
                        merge_scan_take(&r.open, &r.openD, v.seq, d2);
                        continue;
                    }
                    if (t != v.seq) continue;   // pending or merged: not a vertex
                }
                merge_scan_take(&r.best, &r.bestD, v.seq, d2);
            }
        }
    return r;
}

// Point i (state cur < 0, position q) after its scan r: true when it is final afterwards
template <typename St>
AVR_HD bool merge_decide(const MergeView &mv, int i, int cur, const MergeRec &q, const MergeScan &r, St &st) {
    const int seq = mv.v0 + i;
    if (r.best >= 0) {
        // an undecided point behind the best vertex in key order cannot become the target
        if (r.open < 0 || r.bestD < r.openD || (r.bestD == r.openD && r.best < r.open)) {
            st.store(i, r.best);
            return true;
        }
        if (cur == kMergeUndecided) st.store(i, kMergePending);
        return false;
    }
    if (r.open >= 0) return false;
    int pv = mv.prev[i];
    if (pv >= mv.v0) {
        pv = st.load(pv - mv.v0);
        if (pv < 0) return false;   // the predecessor's vertex is not known yet
    }
    int target = seq;
    if (pv >= 0) {
        const MergeRec u = mv.ent[pv];
        const float dx = u.x - q.x, dy = u.y - q.y, dz = u.z - q.z;
        if (dx * dx + dy * dy + dz * dz <= mv.r2) target = pv;
    }
    st.store(i, target);
    return true;
}

// One step of point i by one lane. True when the point is final afterwards.
template <typename St>
AVR_HD bool merge_step(const MergeView &mv, int i, St &st) {
    const int cur = st.load(i);
    if (cur >= 0) return true;
    const MergeRec q = mv.ent[mv.v0 + i];
    const MergeScan r = merge_scan(mv, mv.v0 + i, q, st, 0, 1);
    return merge_decide(mv, i, cur, q, r, st);
}

// The states of the round before (load) and of this one (store): the host's synchronous rounds
struct MergeStateHost {
    const int *before;
    int *now;
    int load(int i) const { return before[i]; }
    void store(int i, int v) { now[i] = v; }
};

// Final states -> vertex ids: a new point's id is V0 + the number of new points before it
inline void merge_ids(const int *state, int v0, int n, int *ids) {
    std::vector<int> rank((size_t)n);
    int news = 0;
    for (int i = 0; i < n; ++i) {
        rank[(size_t)i] = news;
        news += state[i] == v0 + i;
    }
    for (int i = 0; i < n; ++i) ids[i] = state[i] < v0 ? state[i] : v0 + rank[(size_t)(state[i] - v0)];
}

// The host grid over a call's entities. Build() returns a message on a bad argument, else
// null; counts and start vertices are the caller's to range-check (avr_graph_add_walks_from).
class MergeGrid {
  public:
    const char *Build(float radius, size_t v0, const float *vxyz, long long n_walks, int max_depth, const float *points,
                      const int *counts, const int *start) {
        long long n = 0;
        for (long long w = 0; w < n_walks; ++w) n += counts[w];
        if ((long long)v0 + n > 0x7fffffff) return "graph merge: more than 2^31 - 1 vertices and points";
        v0_ = (int)v0;
        n_ = (int)n;
        const size_t E = v0 + (size_t)n;
        ent_.resize(E);
        prev_.resize((size_t)n);
        first_.resize((size_t)n_walks + 1);
        for (size_t v = 0; v < v0; ++v) ent_[v] = {vxyz[3 * v], vxyz[3 * v + 1], vxyz[3 * v + 2], (int)v};
        int seq = v0_;
        for (long long w = 0; w < n_walks; ++w) {
            first_[(size_t)w] = seq - v0_;
            const float *p = points + (size_t)w * max_depth * 3;
            for (int j = 0; j < counts[w]; ++j, ++seq) {
                ent_[(size_t)seq] = {p[3 * j], p[3 * j + 1], p[3 * j + 2], seq};
                prev_[(size_t)(seq - v0_)] = j > 0 ? seq - 1 : (start ? start[w] : -1);
            }
        }
        first_[(size_t)n_walks] = n_;
        for (int a = 0; a < 3; ++a) {
            bmin_[a] = 0;
            dim_[a] = 1;
        }
        inv_ = 1.0 / (double)radius;
        r2_ = radius * radius;   // Sqr(nodeRadius), as Builder's
        reach_ = std::sqrt((double)r2_) * (1.0 + 1e-6) + 1e-22;
        rec_.assign(ent_.begin(), ent_.end());
        work_.clear();
        start_.assign(2, 0);
        if (E == 0) return nullptr;
        double bmin[3], bmax[3];
        for (int a = 0; a < 3; ++a) bmin[a] = bmax[a] = (&ent_[0].x)[a];
        for (size_t e = 0; e < E; ++e)
            for (int a = 0; a < 3; ++a) {
                const float x = (&ent_[e].x)[a];
                if (!std::isfinite(x)) return "graph merge: non-finite coordinate";
                bmin[a] = std::min(bmin[a], (double)x);
                bmax[a] = std::max(bmax[a], (double)x);
            }
        double cell = (double)radius;
        long long dim[3];
        while (true) {   // Index::Build's sizing
            bool fits = true;
            long long cells = 1;
            inv_ = 1.0 / cell;
            for (int a = 0; a < 3 && fits; ++a) {
                const double d = index_cell_coord(bmax[a], bmin[a], inv_) + 1.0;
                fits = d <= (double)kIndexCellBudget;
                dim[a] = fits ? (long long)d : 0;
                cells *= dim[a];
                fits = fits && cells <= kIndexCellBudget;
            }
            if (fits) break;
            cell *= 2.0;
        }
        for (int a = 0; a < 3; ++a) {
            bmin_[a] = bmin[a];
            dim_[a] = (int)dim[a];
        }
        const size_t cells = (size_t)dim_[0] * dim_[1] * dim_[2];
        std::vector<int> cellOf(E);
        start_.assign(cells + 1, 0);
        for (size_t e = 0; e < E; ++e) {
            int c[3];
            for (int a = 0; a < 3; ++a) {
                const double k = index_cell_coord((double)(&ent_[e].x)[a], bmin_[a], inv_);
                c[a] = k < 0.0 ? 0 : (k > (double)(dim_[a] - 1) ? dim_[a] - 1 : (int)k);
            }
            cellOf[e] = (c[2] * dim_[1] + c[1]) * dim_[0] + c[0];
            ++start_[(size_t)cellOf[e] + 1];
        }
        for (size_t c = 0; c < cells; ++c) start_[c + 1] += start_[c];
        std::vector<int> fill(start_.begin(), start_.end() - 1);
        for (size_t e = 0; e < E; ++e) rec_[(size_t)fill[(size_t)cellOf[e]]++] = ent_[e];
        // the points in sorted order: neighbouring lanes scan the same cells
        work_.reserve((size_t)n);
        for (size_t s = 0; s < E; ++s)
            if (rec_[s].seq >= v0_) work_.push_back(rec_[s].seq - v0_);
        return nullptr;
    }

    MergeView View() const {
        MergeView v{};
        v.rec = rec_.data();
        v.ent = ent_.data();
        v.cell_start = start_.data();
        v.prev = prev_.data();
        for (int a = 0; a < 3; ++a) {
            v.bmin[a] = bmin_[a];
            v.dim[a] = dim_[a];
        }
        v.inv_cell = inv_;
        v.reach = reach_;
        v.v0 = v0_;
        v.n = n_;
        v.r2 = r2_;
        return v;
    }

    // Synchronous rounds on the host until every point is final: state[i] = the seq of point
    // i's vertex. False when a round finalised nothing (cannot happen: see the header).
    bool Assign(std::vector<int> *state, int *rounds) const {
        const MergeView mv = View();
        state->assign((size_t)n_, kMergeUndecided);
        std::vector<int> before(*state), work(work_), left;
        int r = 0;
        while (!work.empty()) {
            MergeStateHost st{before.data(), state->data()};
            left.clear();
            for (int i : work)
                if (!merge_step(mv, i, st)) left.push_back(i);
            ++r;
            if (left.size() == work.size()) return false;
            for (int i : work) before[(size_t)i] = (*state)[(size_t)i];
            work.swap(left);
        }
        *rounds = r;
        return true;
    }

    int NumPoints() const { return n_; }
    int NumExisting() const { return v0_; }
    size_t NumCells() const { return start_.size() - 1; }
    const std::vector<int> &Work() const { return work_; }
    // walk w's points are first[w] .. first[w + 1] - 1
    const std::vector<int> &WalkFirst() const { return first_; }

  private:
    std::vector<MergeRec> rec_, ent_;
    std::vector<int> start_, prev_, work_, first_;
    double bmin_[3] = {0, 0, 0}, inv_ = 1, reach_ = 0;
    int dim_[3] = {1, 1, 1};
    int v0_ = 0, n_ = 0;
    float r2_ = 0;
};

}  // namespace graph
}  // namespace avr
