/*
 * align_map.h -- the host side of the alignment report (include/gdg.h, gdg_block_align_rows): the reference list's validation, the rule by
 * which a list replaces the one in force, and the list cut into the pieces a launch takes by value.  Plain C++, no device and no context:
 * tests/native/align_check.cpp drives it under AddressSanitizer and UBSan.
 */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#define GDG_ALIGN_BLOCK 8192                  /* L: the samples of a block = the length of the transform */
#define GDG_ALIGN_MAX_LAG 2048                /* 1 <= M <= 2048: the central L - 2M samples of the reference are at least half the block */
#define GDG_ALIGN_PAIRS 240                   /* measured ports per launch: the pairs travel in the kernel's arguments */

/* what the kernel is given by value: workgroup y of a launch measures port[y] against ref[y] */
struct gdg_align_pairs {
    int n, max_lag;
    int port[GDG_ALIGN_PAIRS], ref[GDG_ALIGN_PAIRS];
};

enum { ALIGN_OK = 0, ALIGN_COUNT = 1, ALIGN_NULL = 2, ALIGN_REF = 3, ALIGN_LAG = 4 };

/* n_ports >= 1 entries, each -1 (not measured) or a port of the same list; 1 <= max_lag <= 2048.  *bad: the first offending entry, -1 when
 * the list as a whole (or the lag) is refused */
static inline int align_map_check(const int *ref, int n_ports, int max_lag, int *bad) {
    *bad = -1;
    if (n_ports < 1) return ALIGN_COUNT;
    if (!ref) return ALIGN_NULL;
    if (max_lag < 1 || max_lag > GDG_ALIGN_MAX_LAG) return ALIGN_LAG;
    for (int p = 0; p < n_ports; p++)
        if (ref[p] < -1 || ref[p] >= n_ports) { *bad = p; return ALIGN_REF; }
    return ALIGN_OK;
}

/* whole or not at all: a refused list leaves the map and the lag in force as they are */
static inline int align_map_replace(std::vector<int> &map, int &lag, const int *ref, int n_ports, int max_lag, int *bad) {
    const int rc = align_map_check(ref, n_ports, max_lag, bad);
    if (rc != ALIGN_OK) return rc;
    map.assign(ref, ref + n_ports);
    lag = max_lag;
    return ALIGN_OK;
}

/* the measured ports of a checked list, in ascending order, GDG_ALIGN_PAIRS to a piece; `skip`: a port that is neither measured nor
 * referenced in this call (a shard's metronome row when the shard does not run it), -1 for none */
static inline std::vector<gdg_align_pairs> align_map_pieces(const std::vector<int> &map, int max_lag, int skip = -1) {
    std::vector<gdg_align_pairs> out;
    for (size_t p = 0; p < map.size(); p++) {
        if (map[p] < 0 || (int)p == skip || map[p] == skip) continue;
        if (out.empty() || out.back().n == GDG_ALIGN_PAIRS) {
            out.push_back(gdg_align_pairs());
            out.back().n = 0;
            out.back().max_lag = max_lag;
            for (int i = 0; i < GDG_ALIGN_PAIRS; i++) out.back().port[i] = out.back().ref[i] = 0;
        }
        gdg_align_pairs &q = out.back();
        q.port[q.n] = (int)p;
        q.ref[q.n] = map[p];
        q.n++;
    }
    return out;
}
