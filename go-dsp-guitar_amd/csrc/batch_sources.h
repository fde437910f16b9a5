/*
 * batch_sources.h -- the source map of a batch job (gdg_batch_set_sources): which channel's input entry every channel reads.
 * Plain host code without a device call or a context, so that a stand-alone program can drive it (tests/native/sources_check.cpp):
 * the validation of a map, readers -> roots, and per root the rows it feeds (the list a step's fan-out descriptors are made from).
 */
#ifndef GDG_BATCH_SOURCES_H
#define GDG_BATCH_SOURCES_H
#include <cstddef>
#include <vector>

/* why a map is refused; `channel` of sources_check names the first offender */
enum { SOURCES_OK = 0, SOURCES_WRONG_N, SOURCES_OUT_OF_RANGE, SOURCES_CHAIN };

/* source[c] == c: a root (reads its own entry); anything else: a reader, whose source must be a root.  n must be the channel count. */
static inline int sources_check(const int *source, int n, int channels, int *channel) {
    if (channel) *channel = -1;
    if (!source || n != channels || n <= 0) return SOURCES_WRONG_N;
    for (int c = 0; c < n; c++)
        if (source[c] < 0 || source[c] >= n) { if (channel) *channel = c; return SOURCES_OUT_OF_RANGE; }
    for (int c = 0; c < n; c++)
        if (source[source[c]] != source[c]) { if (channel) *channel = c; return SOURCES_CHAIN; }
    return SOURCES_OK;
}

static inline bool sources_have_reader(const std::vector<int> &source) {
    for (size_t c = 0; c < source.size(); c++) if (source[c] != (int)c) return true;
    return false;
}

/* the root of channel c under a map (an empty map: every channel its own) */
static inline int sources_root(const std::vector<int> &source, int c) { return source.empty() ? c : source[(size_t)c]; }

/* Readers per root, as offsets into one list: the readers of root r are list[first[r] .. first[r + 1]), in channel order; a reader's own
 * range is empty.  A valid map is assumed (sources_check). */
struct SourceFans {
    std::vector<int> first, list;
    int fan(int root) const { return first[(size_t)root + 1] - first[(size_t)root]; }      /* rows fed beside the root's own */
    const int *readers(int root) const { return list.data() + first[(size_t)root]; }
};
static inline SourceFans sources_fans(const std::vector<int> &source) {
    const size_t n = source.size();
    SourceFans f;
    f.first.assign(n + 1, 0);
    for (size_t c = 0; c < n; c++) if (source[c] != (int)c) f.first[(size_t)source[c] + 1]++;
    for (size_t r = 0; r < n; r++) f.first[r + 1] += f.first[r];
    f.list.assign((size_t)f.first[n], 0);
    std::vector<int> at(f.first.begin(), f.first.end() - 1);
    for (size_t c = 0; c < n; c++) if (source[c] != (int)c) f.list[(size_t)at[(size_t)source[c]]++] = (int)c;
    return f;
}
#endif
