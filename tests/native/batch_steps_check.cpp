/*
 * batch_steps_check.cpp -- the step plan of the batch block loop (csrc/batch_steps.h) without HIP.  For windows W of 1, 2, 4, 8 and 16 blocks,
 * every job of 1 to 64 blocks and every slice [origin, origin + n) inside the job:
 *   - slice_steps gives the list THE RULE IT REPLACED gave -- that rule, the step rule and the loop that cut a slice as they stood inside
 *     batch_block_loop (api_batch.cpp), is copied here verbatim (old_job_step, old_slice_steps; offsets in samples, blocks of 8192);
 *   - the steps cover the slice exactly, without a gap or an overlap, and every w is a power of two <= W;
 *   - every step of a slice lies inside one step of the whole job, and ends where that step ends or where the slice does;
 *   - the whole job as one slice gives the sequence job_step walks.
 * And three sequences derived by hand from the rule: a job of 29 blocks at W = 8 (head 2, 4; two whole windows; tail 4, 2, 1), the same job cut
 * as 13 + 16, and a job of 5 blocks at W = 4 cut as 3 + 2.  Built by tests/test_batch_steps_host.py.
 */
#include "batch_steps.h"

#include <algorithm>
#include <cstdio>
#include <initializer_list>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

/* ---- the rule it replaced, verbatim ---- */
static void old_job_step(size_t job, int W, size_t p, size_t *first, int *w) {
    const size_t head = (W >= 8 && job >= (size_t)3 * W) ? (size_t)(W / 4 + W / 2) : 0;
    if (head && p < (size_t)(W / 4)) { *first = 0; *w = W / 4; return; }
    if (head && p < head) { *first = (size_t)(W / 4); *w = W / 2; return; }
    const size_t full = (job - head) / (size_t)W * (size_t)W;
    if (p - head < full) { *first = head + (p - head) / (size_t)W * (size_t)W; *w = W; return; }
    size_t off = head + full;
    int k = W;
    for (;;) {
        while ((size_t)k > job - off) k >>= 1;
        if (p < off + (size_t)k || k <= 1) { *first = off; *w = k; return; }
        off += (size_t)k;
    }
}

struct OldStep { size_t off; int w; };
struct OldLoop { size_t job_blocks, origin_blocks; };

static std::vector<OldStep> old_slice_steps(const OldLoop &p, size_t length, int W) {
    const int B = 8192;
    std::vector<OldStep> steps;
    for (size_t off = 0; off < length;) {
        const size_t at = p.origin_blocks + off / B, end = p.origin_blocks + length / B;
        size_t first = 0;
        int w1 = 1, w = 1;
        old_job_step(p.job_blocks, W, at, &first, &w1);
        const size_t room = std::min(first + (size_t)w1, end) - at;
        while ((size_t)w * 2 <= room) w *= 2;
        steps.push_back({ off, w });
        off += (size_t)w * B;
    }
    return steps;
}

static bool widths_are(const std::vector<SliceStep> &steps, std::initializer_list<int> want) {
    if (steps.size() != want.size()) return false;
    size_t i = 0, off = 0;
    for (int w : want) {
        if (steps[i].w != w || steps[i].off != off) return false;
        off += (size_t)w;
        i++;
    }
    return true;
}

int main() {
    long cases = 0, cut_short = 0, heads = 0;
    for (int W : { 1, 2, 4, 8, 16 })
        for (size_t job = 1; job <= 64; job++) {
            const std::vector<SliceStep> whole = slice_steps(job, 0, job, W);
            /* one slice: the sequence job_step walks */
            size_t at = 0, i = 0;
            while (at < job) {
                size_t first = 0;
                int w = 0;
                job_step(job, W, at, &first, &w);
                CHECK(i < whole.size() && first == at && whole[i].off == at && whole[i].w == w);
                at += (size_t)w;
                i++;
            }
            CHECK(at == job && i == whole.size());
            if (whole.size() > 1 && whole[0].w < whole[1].w) heads++;
            for (size_t origin = 0; origin < job; origin++)
                for (size_t n = 1; origin + n <= job; n++) {
                    const std::vector<SliceStep> got = slice_steps(job, origin, n, W);
                    /* against the rule it replaced */
                    const std::vector<OldStep> old = old_slice_steps({ job, origin }, n * 8192, W);
                    CHECK(got.size() == old.size());
                    for (size_t k = 0; k < got.size() && k < old.size(); k++) CHECK(got[k].off * 8192 == old[k].off && got[k].w == old[k].w);
                    /* cover */
                    size_t next = 0;
                    for (const SliceStep &s : got) {
                        CHECK(s.off == next && s.w >= 1 && s.w <= W && (s.w & (s.w - 1)) == 0);
                        next += (size_t)s.w;
                    }
                    CHECK(next == n);
                    /* nesting */
                    for (size_t k = 0; k < got.size(); k++) {
                        const SliceStep &s = got[k];
                        const size_t b0 = origin + s.off, b1 = b0 + (size_t)s.w;
                        size_t j = 0;
                        while (j < whole.size() && whole[j].off + (size_t)whole[j].w <= b0) j++;
                        CHECK(j < whole.size());
                        if (j >= whole.size()) continue;
                        const size_t j0 = whole[j].off, j1 = j0 + (size_t)whole[j].w;
                        CHECK(j0 <= b0 && b1 <= j1);
                        /* the run of slice steps inside one step of the job ends where that step ends, or where the slice does: a step that
                         * ends at neither is followed by a smaller one inside the same step of the job (7 blocks of a window: 4, 2, 1) */
                        const bool run_goes_on = k + 1 < got.size() && origin + got[k + 1].off + (size_t)got[k + 1].w <= j1 && got[k + 1].w < s.w;
                        CHECK(b1 == j1 || b1 == origin + n || run_goes_on);
                        if (b1 == origin + n && b1 != j1) cut_short++;
                    }
                    cases++;
                }
        }
    CHECK(cut_short > 0 && heads > 0);                                           /* slices did end inside a job's step, and long jobs did open small */
    /* derived by hand: 29 >= 3 * 8, so the head is 2, 4; (29 - 6) / 8 = 2 whole windows; 7 blocks are left: 4, 2, 1 */
    CHECK(widths_are(slice_steps(29, 0, 29, 8), { 2, 4, 8, 8, 4, 2, 1 }));
    /* 13 blocks: 2, 4, then the window [6, 14) holds 7 of the slice's blocks: 4, 2, 1 */
    CHECK(widths_are(slice_steps(29, 0, 13, 8), { 2, 4, 4, 2, 1 }));
    /* 16 blocks from 13: the last block of [6, 14), the window [14, 22), the tail */
    CHECK(widths_are(slice_steps(29, 13, 16, 8), { 1, 8, 4, 2, 1 }));
    /* 5 blocks at W = 4: the job steps 4, 1; blocks [0, 3) lie in [0, 4): 2, 1; block 3 ends that step, block 4 is the tail */
    CHECK(widths_are(slice_steps(5, 0, 3, 4), { 2, 1 }));
    CHECK(widths_are(slice_steps(5, 3, 2, 4), { 1, 1 }));
    /* the pieces of a step's download: four from 4 blocks and 8 encoded rows on */
    CHECK(step_pieces(4, 8) == 4 && step_pieces(16, 515) == 4 && step_pieces(2, 8) == 1 && step_pieces(4, 7) == 1 && step_pieces(1, 1) == 1);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("OK step plan; %ld cases\n", cases);
    return 0;
}
