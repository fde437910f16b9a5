/*
 * trim_check.cpp -- csrc/trim.h driven on the host, without HIP: the planner against the known answers of include/gdg.h (a silent port, the
 * max_gain cap, a NaN record, a bad target, blocks == 0), the gain list's checks, and the product's single rounding.  With a table file
 * as argument: lines "x_bits g_bits y_bits" (hex float64 bit patterns, made by the numpy restatement) held against gdg_trim_apply.
 * Built with -fsanitize=address,undefined by tests/test_trim_host.py; prints "OK ..." and returns 0, or says what differs.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "trim.h"

struct Rec { double true_peak; uint32_t position, overs; };      /* gdg_block_true_peak's layout: 16 bytes */
static_assert(sizeof(Rec) == 16, "two doubles wide");

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static std::vector<Rec> records(const std::vector<std::vector<double>> &peaks) {
    std::vector<Rec> out;
    for (auto &row : peaks) for (double v : row) out.push_back(Rec{ v, 7u, 9u });
    return out;
}
static int plan(const std::vector<Rec> &rec, int ports, size_t blocks, double target, double max_gain, double *gain, int *bad) {
    return gdg_trim_plan(rec.empty() ? nullptr : &rec[0].true_peak, 2, ports, blocks, target, max_gain, gain, bad);
}
static bool near(double a, double b) { return fabs(a - b) <= 1e-9 * fabs(b); }

static uint64_t bits_of(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }
static double from_bits(uint64_t b) { double v; memcpy(&v, &b, 8); return v; }

int main(int argc, char **argv) {
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
        unsigned long long xb, gb, yb;
        size_t rows = 0;
        while (fscanf(f, "%llx %llx %llx", &xb, &gb, &yb) == 3) {
            const double y = gdg_trim_apply(from_bits(xb), from_bits(gb));
            if (bits_of(y) != yb) { printf("row %zu: %a * %a = %a, the table says %a\n", rows, from_bits(xb), from_bits(gb), y, from_bits(yb)); failures++; }
            rows++;
        }
        fclose(f);
        if (failures) return 1;
        printf("OK %zu rows\n", rows);
        return 0;
    }
    const double T = 0.891250938, nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    int bad = -1;
    /* the header's known answers: the port's largest block counts, wherever it lies; a silent port; the cap */
    {
        auto rec = records({ { 0.1, 0.5, 0.3 }, { 2.0, 0.0, 1.0 }, { 0.0, 0.0, 0.0 } });
        double gain[3] = { -1, -1, -1 };
        CHECK(plan(rec, 3, 3, T, 4.0, gain, &bad) == GDG_TRIM_PLAN_OK);
        CHECK(near(gain[0], 1.782501876) && near(gain[1], 0.445625469) && gain[2] == 1.0);
        CHECK(gain[0] == T / 0.5 && gain[1] == T / 2.0);
    }
    {
        auto rec = records({ { 0.01 } });
        double gain[1] = { -1 };
        CHECK(plan(rec, 1, 1, T, 4.0, gain, &bad) == GDG_TRIM_PLAN_OK && gain[0] == 4.0);
        CHECK(plan(rec, 1, 1, T, 100.0, gain, &bad) == GDG_TRIM_PLAN_OK && gain[0] == T / 0.01);
    }
    /* a NaN record names its port and writes nothing */
    {
        auto rec = records({ { 0.5, 0.5 }, { 0.25, nan }, { nan, 0.1 } });
        double gain[3] = { -1, -1, -1 };
        bad = -1;
        CHECK(plan(rec, 3, 2, T, 4.0, gain, &bad) == GDG_TRIM_PLAN_NAN && bad == 1);
        CHECK(gain[0] == -1 && gain[1] == -1 && gain[2] == -1);
    }
    /* target and max_gain: finite and greater than 0 */
    {
        auto rec = records({ { 0.5 } });
        double gain[1] = { -1 };
        for (double t : { 0.0, -1.0, nan, inf, -inf }) CHECK(plan(rec, 1, 1, t, 4.0, gain, &bad) == GDG_TRIM_PLAN_TARGET);
        for (double m : { 0.0, -1.0, nan, inf, -inf }) CHECK(plan(rec, 1, 1, T, m, gain, &bad) == GDG_TRIM_PLAN_MAX_GAIN);
        CHECK(gain[0] == -1);
        CHECK(gdg_trim_plan(&rec[0].true_peak, 2, 1, 1, T, 4.0, nullptr, &bad) == GDG_TRIM_PLAN_ARGS);
        CHECK(gdg_trim_plan(nullptr, 2, 1, 1, T, 4.0, gain, &bad) == GDG_TRIM_PLAN_ARGS);
        CHECK(gdg_trim_plan(&rec[0].true_peak, 2, -1, 1, T, 4.0, gain, &bad) == GDG_TRIM_PLAN_ARGS);
    }
    /* blocks == 0: nothing was rendered, every gain 1; no record is read (records may be NULL); ports == 0 writes nothing */
    {
        double gain[2] = { -1, -1 };
        CHECK(gdg_trim_plan(nullptr, 2, 2, 0, T, 4.0, gain, &bad) == GDG_TRIM_PLAN_OK && gain[0] == 1.0 && gain[1] == 1.0);
        gain[0] = -1;
        CHECK(gdg_trim_plan(nullptr, 2, 0, 5, T, 4.0, gain, &bad) == GDG_TRIM_PLAN_OK && gain[0] == -1);
    }
    /* the gain list's checks */
    {
        const double ok[4] = { 0.5, -1.0, 0.0, 3.0 }, one[3] = { 1.0, 1.0, 1.0 }, with_nan[3] = { 1.0, nan, inf }, with_inf[2] = { 1.0, -inf };
        CHECK(gdg_trim_first_nonfinite(ok, 4) == -1 && gdg_trim_first_nonfinite(with_nan, 3) == 1 && gdg_trim_first_nonfinite(with_inf, 2) == 1);
        CHECK(gdg_trim_first_nonfinite(ok, 0) == -1);
        CHECK(gdg_trim_all_unit(one, 3) && !gdg_trim_all_unit(ok, 4) && gdg_trim_all_unit(ok, 0));
        const double minus_zero_gain[1] = { -1.0 };
        CHECK(!gdg_trim_all_unit(minus_zero_gain, 1));
    }
    /* the product: rounded once; 1.0 is the identity on every finite sample, a power of two is exact, -1 flips the sign alone */
    {
        const double xs[] = { 0.0, -0.0, 1e-5, 2e-5, -0.7, 1.0, -1.0, 1.0 - 0x1p-53, 0x1p-1074, 1e308, 0.1 };
        for (double x : xs) {
            CHECK(bits_of(gdg_trim_apply(x, 1.0)) == bits_of(x));
            CHECK(bits_of(gdg_trim_apply(x, -1.0)) == (bits_of(x) ^ 0x8000000000000000ull));
        }
        CHECK(gdg_trim_apply(2e-5, 0.5) == 1e-5);
        CHECK(gdg_trim_apply(0.1, 3.0) == 0.30000000000000004);          /* the rounded product, not the exact 0.3 */
        CHECK(gdg_trim_apply(0.7, 0.0) == 0.0 && bits_of(gdg_trim_apply(-0.7, 0.0)) == 0x8000000000000000ull);
    }
    if (failures) return 1;
    printf("OK\n");
    return 0;
}
