/*
 * batch_steps.h -- the step plan of the batch block loop (api_batch.cpp): which steps of how many blocks a job runs in (job_step), where a
 * slice of the job cuts them (slice_steps), and in how many pieces a step comes down (step_pieces).  It is what makes a sliced job
 * byte-identical to the one-call job.  Pure host arithmetic in whole blocks: no HIP header is needed to compile this file
 * (tests/native/batch_steps_check.cpp holds it against the loop it replaced and against sequences derived by hand).
 */
#ifndef GDG_BATCH_STEPS_H
#define GDG_BATCH_STEPS_H

#include <stddef.h>
#include <vector>

/* The step rule: the step [first, first + w) that holds block p of a job of `job` blocks in windows of W.
 * A long job opens with a quarter window and a half window: the device has nothing to do until the first step's bytes are gathered and
 * uploaded (16 blocks of 512 files: 1.9 + 2.4 ms), and what it computes first comes down and is scattered while nothing else waits for the
 * host; each step's upload fits behind the step before.  Then whole windows, then a tail of W/2, W/4 .. 1 (the last download and scatter
 * are a quarter step's).  Window sizes only change the time blocking, never a sample (tests/test_gpu_window.py). */
static inline void job_step(size_t job, int W, size_t p, size_t *first, int *w) {
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

/* a step of a slice: `w` blocks from block `off` of the slice on */
struct SliceStep { size_t off; int w; };

/* The steps of the slice [origin_blocks, origin_blocks + slice_blocks) of a job of job_blocks blocks.  A slice steps where the whole job
 * does (job_step): a step ends where the job's step ends (or the slice does), so that the windows -- and with them what the units keep
 * beyond the samples, the convolution's two history halves -- are those of the job run as one slice wherever the slicing allows it */
static inline std::vector<SliceStep> slice_steps(size_t job_blocks, size_t origin_blocks, size_t slice_blocks, int W) {
    std::vector<SliceStep> steps;
    const size_t end = origin_blocks + slice_blocks;
    for (size_t off = 0; off < slice_blocks;) {
        const size_t at = origin_blocks + off;
        size_t first = 0;
        int w1 = 1, w = 1;
        job_step(job_blocks, W, at, &first, &w1);
        const size_t step_end = first + (size_t)w1, room = (step_end < end ? step_end : end) - at;
        while ((size_t)w * 2 <= room) w *= 2;
        steps.push_back({ off, w });
        off += (size_t)w;
    }
    return steps;
}

/* A step of w blocks and enc_rows encoded rows comes down in this many pieces of whole rows, an event behind each: the scatter of piece c
 * runs while piece c + 1 is on the bus -- the run's tail (last download, then last scatter) and its head are that much shorter; in between
 * the device sets the pace either way. */
static inline int step_pieces(int w, int enc_rows) { return (w >= 4 && enc_rows >= 8) ? 4 : 1; }

#endif
