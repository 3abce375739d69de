// The 0-dimensional persistence of the basins of a mesh (tn_mesh_hotspots.hip exports it as tn_basin_persistence; DESIGN.md "Thermal
// hot spots"; include/thermonerf_hip.h defines every output): the merge of the basin graph in ascending pass rank, on the host, in
// integers only.  Plain C++: no HIP, no device pointer, and no allocation beyond the two index arrays of merge() — the order of the
// saddles and the union-find over the basins.  O(S log S) for the one sort; the loop itself is S finds with path halving.
//
//   saddles        rows (a, b, pass_vertex, pass_rank) as tn_mesh_peaks writes them, in ascending (a, b)
//   a BATCH        all saddles of one pass_rank, taken in ascending row (which is ascending (a, b))
//   a component    its representative is the member whose peak has the smallest rank (ranks are distinct: the eldest is unique)
//   a saddle that joins two components kills the representative with the larger peak rank: death_saddle[it] = the row
//   after the batch parent[d] = find(d) for every basin d that died in it: the eldest of everything joined at that pass vertex
//   a basin that never dies keeps death_saddle = parent = -1: one per connected component of the basin graph
#pragma once
#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

namespace tn {

enum { kPersistenceOk = 0, kPersistenceBadRow = 1, kPersistenceNoMemory = 2 };

namespace detail {
inline int32_t find_root(int32_t *up, int32_t x) {
    while (up[x] != x) {
        up[x] = up[up[x]];  // path halving
        x = up[x];
    }
    return x;
}
}  // namespace detail

// basin_rank [B]: the rank of every basin's peak; saddles [S, 4]; death_saddle, parent [B].  kPersistenceBadRow: a row names a basin
// outside [0, B) or the same basin twice — nothing is then written
inline int merge(const int32_t *basin_rank, int64_t num_basins, const int32_t *saddles, int64_t num_saddles, int32_t *death_saddle,
                 int32_t *parent) {
    for (int64_t s = 0; s < num_saddles; ++s) {
        const int64_t a = saddles[4 * s], b = saddles[4 * s + 1];
        if (a < 0 || a >= num_basins || b < 0 || b >= num_basins || a == b) return kPersistenceBadRow;
    }
    std::vector<int32_t> order, up;
    try {
        order.resize((size_t)num_saddles);
        up.resize((size_t)num_basins);
    } catch (const std::bad_alloc &) {
        return kPersistenceNoMemory;
    }
    for (int64_t b = 0; b < num_basins; ++b) up[(size_t)b] = (int32_t)b, death_saddle[b] = parent[b] = -1;
    for (int64_t s = 0; s < num_saddles; ++s) order[(size_t)s] = (int32_t)s;
    std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        const int32_t px = saddles[4 * (int64_t)x + 3], py = saddles[4 * (int64_t)y + 3];
        return px != py ? px < py : x < y;
    });
    for (int64_t first = 0; first < num_saddles;) {
        const int32_t pass = saddles[4 * (int64_t)order[(size_t)first] + 3];
        int64_t end = first;
        for (; end < num_saddles && saddles[4 * (int64_t)order[(size_t)end] + 3] == pass; ++end) {
            const int32_t row = order[(size_t)end];
            const int32_t ra = detail::find_root(up.data(), saddles[4 * (int64_t)row]);
            const int32_t rb = detail::find_root(up.data(), saddles[4 * (int64_t)row + 1]);
            order[(size_t)end] = -1;  // the row is spent: its place now remembers who died by it
            if (ra == rb) continue;
            const bool a_elder = basin_rank[ra] < basin_rank[rb] || (basin_rank[ra] == basin_rank[rb] && ra < rb);
            const int32_t elder = a_elder ? ra : rb, younger = a_elder ? rb : ra;
            up[(size_t)younger] = elder;
            death_saddle[younger] = row;
            order[(size_t)end] = younger;
        }
        for (int64_t k = first; k < end; ++k) {
            const int32_t d = order[(size_t)k];
            if (d >= 0) parent[d] = detail::find_root(up.data(), d);
        }
        first = end;
    }
    return kPersistenceOk;
}

}  // namespace tn
