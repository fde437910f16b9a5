/*
 * delivered_spans_check.cpp -- the block spans of the delivered rows' records (include/gdg.h, DELIVERED RECORDS) as a program of its own: the
 * batch loop cuts a step's delivered rows into its session blocks' samples with deliver_ratio_step (csrc/deliver.h); here those spans are
 * held against N(s) = gdg_batch_out_samples(factor, up, down, 0, s) = gdg_deliver_samples -- and that against a plain 128-bit ceil(s L / M) --
 * for the factors 1, 2, 4 and the ratios 1/1, 147/160, 160/147, 1/2, 2/1 over 64 blocks, however the job is cut into slices and steps.
 * Pure host arithmetic: builds with g++ alone, also under -fsanitize=address,undefined.
 */
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "deliver.h"

static const int BLOCKS = 64, B = 8192;

static unsigned long long plain_first(unsigned long long s, int L, int M) {
    const unsigned __int128 num = (unsigned __int128)s * (unsigned)L + (unsigned)(M - 1);
    return (unsigned long long)(num / (unsigned)M);
}

/* the spans of a step of w blocks `off` samples into a slice that begins at `pos`, as api_batch.cpp makes them */
static std::vector<unsigned long long> step_spans(size_t w, size_t off, size_t pos, int R, int L, int M) {
    std::vector<unsigned long long> span;
    for (size_t j = 0; j <= w; j++) span.push_back((unsigned long long)deliver_ratio_step(j, off, pos, R, L, M, 8, 0).samples);
    return span;
}

int main(void) {
    const int factors[3] = { 1, 2, 4 };
    const int ratios[5][2] = { { 1, 1 }, { 147, 160 }, { 160, 147 }, { 1, 2 }, { 2, 1 } };
    long cases = 0;
    for (int R : factors)
        for (const int *q : ratios) {
            const int L = q[0], M = q[1];
            if (!gdg_deliver_ratio_ok(L, M)) { printf("FAIL ratio %d/%d is not admissible\n", L, M); return 1; }
            /* N(s) against the plain formula, and the job's blocks: lengths of two neighbouring counts between 1024 and 16384 */
            std::vector<unsigned long long> N((size_t)BLOCKS + 1);
            unsigned long long lo = ~0ull, hi = 0;
            for (int k = 0; k <= BLOCKS; k++) {
                N[(size_t)k] = gdg_deliver_samples(R, L, M, 0, (unsigned long long)k * B);
                if (N[(size_t)k] != plain_first((unsigned long long)k * B / (unsigned)R, L, M)) { printf("FAIL N(%d blocks) at %d, %d/%d\n", k, R, L, M); return 1; }
                if (k) {
                    const unsigned long long len = N[(size_t)k] - N[(size_t)k - 1];
                    lo = len < lo ? len : lo;
                    hi = len > hi ? len : hi;
                }
            }
            if (lo < 1024 || hi > 16384 || hi - lo > 1) { printf("FAIL lengths %llu .. %llu at %d, %d/%d\n", lo, hi, R, L, M); return 1; }
            if (L == 1 && M == 1 && (lo != (unsigned long long)(B / R) || hi != lo)) { printf("FAIL a factor alone gives 8192 / R\n"); return 1; }
            /* every cut into two slices, each walked in steps of 1, 2 or 4 blocks (ragged at the slice's end): a step's spans are the job's
             * blocks', counted from the step's first delivered sample, and the steps' samples sum to the slice's, the slices' to the job's */
            for (int cut = 0; cut <= BLOCKS; cut += (cut < 8 || cut > BLOCKS - 8) ? 1 : 7)
                for (int W = 1; W <= 4; W *= 2) {
                    unsigned long long total = 0;
                    const int begin[2] = { 0, cut }, end[2] = { cut, BLOCKS };
                    for (int s = 0; s < 2; s++) {
                        const size_t pos = (size_t)begin[s] * B;
                        unsigned long long slice = 0;
                        for (int at = begin[s]; at < end[s];) {
                            const int w = end[s] - at < W ? end[s] - at : W;
                            const std::vector<unsigned long long> span = step_spans((size_t)w, (size_t)(at - begin[s]) * B, pos, R, L, M);
                            for (int j = 0; j <= w; j++)
                                if (span[(size_t)j] != N[(size_t)(at + j)] - N[(size_t)at]) { printf("FAIL span %d of the step at block %d (cut %d, W %d) at %d, %d/%d\n", j, at, cut, W, R, L, M); return 1; }
                            slice += span[(size_t)w];
                            at += w;
                            cases++;
                        }
                        if (slice != gdg_deliver_samples(R, L, M, pos, (unsigned long long)(end[s] - begin[s]) * B)) { printf("FAIL slice %d of cut %d at %d, %d/%d\n", s, cut, R, L, M); return 1; }
                        total += slice;
                    }
                    if (total != N[(size_t)BLOCKS]) { printf("FAIL the slices of cut %d sum to %llu, the job has %llu\n", cut, total, N[(size_t)BLOCKS]); return 1; }
                }
        }
    printf("OK delivered block spans; %ld step cases\n", cases);
    return 0;
}
