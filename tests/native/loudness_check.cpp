// The loudness planners of csrc/loudness.h as a stand-alone host program (no HIP, no device): the hop count against the plain integer
// formula, the coefficients against the table printed in BS.1770, the launch argument's matrices against A multiplied out one by one, the
// gates of gdg_loudness_plan on hop sums made by hand, and the cap of gdg_loudness_trim_plan.
#include "loudness.h"

#include <stdio.h>
#include <stdlib.h>

static int cases = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        cases++;                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static const double BS1770[10] = { 1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                                   1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621 };

int main() {
    // hops: every cut of a few hundred samples around a hop boundary, at every rate
    const uint32_t rates[] = { 44100, 48000, 96000, 192000 };
    for (uint32_t rate : rates) {
        const uint64_t H = rate / 10;
        for (uint64_t first = 0; first < 3 * H; first += H / 7 + 1)
            for (uint64_t count = 0; count < 2 * H + 300; count += 97) {
                uint64_t n = 0;
                for (uint64_t h = 0; (h + 1) * H <= first + count; h++) if ((h + 1) * H > first) n++;
                CHECK(gdg_loudness_hops_in(rate, first, count) == n);
            }
    }
    CHECK(!gdg_loudness_rate_ok(44101) && !gdg_loudness_rate_ok(0) && !gdg_loudness_rate_ok(7990) && gdg_loudness_rate_ok(8000) && gdg_loudness_rate_ok(44100));

    // the coefficients at 48 kHz are the standard's
    double c[10], worst = 0.0;
    gdg_loudness_coefficients_at(48000.0, c);
    for (int i = 0; i < 10; i++) worst = fmax(worst, fabs(c[i] - BS1770[i]));
    CHECK(worst < 1e-10);
    double alpha = 0.0, beta = 0.0;
    gdg_loudness_hp_delta(48000.0, &alpha, &beta);
    CHECK(fabs(alpha - (1.0 + c[8] + c[9])) < 1e-15 && fabs(beta - (2.0 + c[8])) < 1e-15 && alpha > 0.0 && beta > alpha);

    // P[0] = A^32 and P[k + 1] = P[k]^2, against A applied 32 times to the unit vectors
    const gdg_loudness_params par = gdg_loudness_params_at(48000);
    for (int j = 0; j < 4; j++) {
        double s[4] = { 0.0, 0.0, 0.0, 0.0 };
        s[j] = 1.0;
        for (int n = 0; n < LOUDNESS_CHUNK; n++) {                           // the recurrence at x = 0
            const double y1 = s[0];
            const double s0 = -par.shelf[3] * y1 + s[1], s1 = -par.shelf[4] * y1;
            const double y2 = y1 + s[2];
            const double q0 = s[2] + (s[3] - par.beta * y2), q1 = s[3] - par.alpha * y2;
            s[0] = s0; s[1] = s1; s[2] = q0; s[3] = q1;
        }
        for (int i = 0; i < 4; i++) CHECK(fabs(par.P[0][4 * i + j] - s[i]) < 1e-12);
    }
    for (int k = 0; k + 1 < LOUDNESS_LEVELS; k++) {
        double sq[16];
        gdg_loudness_mat_mul(par.P[k], par.P[k], sq);
        for (int i = 0; i < 16; i++) CHECK(sq[i] == par.P[k + 1][i]);
    }

    // the planner: 3 ports x 100 hops at 48000; power 1 per sample is -0.691 LUFS
    const uint32_t rate = 48000;
    const double H = 4800.0;
    const size_t hops = 100;
    std::vector<double> rec(3 * hops, 0.0);
    for (size_t h = 0; h < hops; h++) {
        rec[h] = H;                                                          // port 0: power 1 throughout
        rec[hops + h] = h < 50 ? H : H * 1e-3;                               // port 1: 30 dB down in the second half: the relative gate drops it
    }                                                                        // port 2: silent
    int port[2] = { 0, 1 };
    double w[2] = { 1.0, 1.41 };
    double integrated = 0.0, momentary = 0.0, shortterm = 0.0;
    long long bad = -1;
    CHECK(gdg_loudness_plan(rec.data(), 3, hops, rate, port, nullptr, 1, &integrated, &momentary, &shortterm, &bad) == GDG_LOUDNESS_PLAN_OK);
    CHECK(fabs(integrated + 0.691) < 1e-12 && fabs(momentary + 0.691) < 1e-12 && fabs(shortterm + 0.691) < 1e-12);
    CHECK(gdg_loudness_plan(rec.data(), 3, hops, rate, port + 1, nullptr, 1, &integrated, &momentary, &shortterm, &bad) == GDG_LOUDNESS_PLAN_OK);
    /* the quiet half is gated; kept are 47 blocks at 1 and the three across the step at 3/4, 1/2 and 1/4 (+ the quiet part): mean 0.97 */
    CHECK(fabs(integrated - (-0.691 + 10.0 * log10((47.0 + 1.5 + 6e-3 / 4.0) / 50.0))) < 1e-9 && fabs(momentary + 0.691) < 1e-12);
    CHECK(gdg_loudness_plan(rec.data(), 3, hops, rate, port, w, 2, &integrated, nullptr, nullptr, &bad) == GDG_LOUDNESS_PLAN_OK);
    /* 2.41 in the first half, 1.00141 in the second, nothing gated: the mean of the 97 blocks, 3 of them across the step */
    CHECK(fabs(integrated - (-0.691 + 10.0 * log10((47.0 * 2.41 + 47.0 * 1.00141 + 1.5 * 2.41 + 1.5 * 1.00141) / 97.0))) < 1e-9);
    int silent = 2;
    CHECK(gdg_loudness_plan(rec.data(), 3, hops, rate, &silent, nullptr, 1, &integrated, &momentary, &shortterm, &bad) == GDG_LOUDNESS_PLAN_OK);
    CHECK(isinf(integrated) && integrated < 0 && isinf(momentary) && isinf(shortterm));
    CHECK(gdg_loudness_plan(rec.data(), 3, 3, rate, port, nullptr, 1, &integrated, &momentary, &shortterm, &bad) == GDG_LOUDNESS_PLAN_OK && isinf(integrated));      // no whole block
    CHECK(gdg_loudness_plan(rec.data(), 3, hops, 44101, port, nullptr, 1, &integrated, nullptr, nullptr, &bad) == GDG_LOUDNESS_PLAN_RATE);
    int outside = 3;
    CHECK(gdg_loudness_plan(rec.data(), 3, hops, rate, &outside, nullptr, 1, &integrated, nullptr, nullptr, &bad) == GDG_LOUDNESS_PLAN_PORT && bad == 0);
    double negative = -1.0;
    CHECK(gdg_loudness_plan(rec.data(), 3, hops, rate, port, &negative, 1, &integrated, nullptr, nullptr, &bad) == GDG_LOUDNESS_PLAN_WEIGHT);
    rec[7] = NAN;
    CHECK(gdg_loudness_plan(rec.data(), 3, hops, rate, port, nullptr, 1, &integrated, nullptr, nullptr, &bad) == GDG_LOUDNESS_PLAN_RECORD && bad == 7);
    rec[7] = H;
    CHECK(gdg_loudness_plan(nullptr, 3, hops, rate, port, nullptr, 1, &integrated, nullptr, nullptr, &bad) == GDG_LOUDNESS_PLAN_ARGS);

    // the trim: port 0 reads -0.691, so -23 asks for 10^(-22.309 / 20); true peaks of 2.0 on port 1 cap it at the ceiling
    double gain[3] = { 0.0, 0.0, 0.0 };
    int capped[3] = { 9, 9, 9 };
    CHECK(gdg_loudness_trim_plan(rec.data(), 3, hops, rate, -23.0, -1.0, nullptr, 0, gain, capped, &bad) == GDG_LOUDNESS_PLAN_OK);
    CHECK(fabs(gain[0] - pow(10.0, -22.309 / 20.0)) < 1e-12 && gain[2] == 1.0 && capped[0] == 0 && capped[1] == 0 && capped[2] == 0);
    std::vector<double> tp(3 * 4 * 2, 0.0);                                  // [3][4] records of (true_peak, position | overs)
    for (int b = 0; b < 4; b++) { tp[(0 * 4 + b) * 2] = 1.0; tp[(1 * 4 + b) * 2] = b == 2 ? 40.0 : 0.5; }
    const double free_gain = gain[1];
    CHECK(gdg_loudness_trim_plan(rec.data(), 3, hops, rate, -23.0, -1.0, tp.data(), 4, gain, capped, &bad) == GDG_LOUDNESS_PLAN_OK);
    CHECK(capped[0] == 0 && capped[1] == 1 && capped[2] == 0 && gain[1] == pow(10.0, -1.0 / 20.0) / 40.0 && gain[1] < free_gain && gain[2] == 1.0);
    tp[2] = NAN;
    gain[0] = 7.0;
    CHECK(gdg_loudness_trim_plan(rec.data(), 3, hops, rate, -23.0, -1.0, tp.data(), 4, gain, capped, &bad) == GDG_LOUDNESS_PLAN_PEAK && bad == 0 && gain[0] == 7.0);
    CHECK(gdg_loudness_trim_plan(rec.data(), 3, hops, rate, NAN, -1.0, nullptr, 0, gain, capped, &bad) == GDG_LOUDNESS_PLAN_TARGET);
    CHECK(gdg_loudness_trim_plan(rec.data(), 3, hops, rate, -23.0, INFINITY, tp.data(), 4, gain, capped, &bad) == GDG_LOUDNESS_PLAN_CEILING);

    printf("OK loudness planners; %d cases; coefficients within %.3e of the BS.1770 table\n", cases, worst);
    return 0;
}
