/* csrc/spectrum_bands.h on the host, under AddressSanitizer and UBSan (tests/test_block_spectrum_abi.py): the validation of an edge list, the
 * first bin of every band and the window table.  No device, no context.
 *   spectrum_check RATE EDGE...   (edges as hexadecimal floats): "OK", k_lo of every edge at RATE, then the 8192 window weights */
#include "spectrum_bands.h"
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

int main(int argc, char **argv) {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    int bad = 0;
    /* the refusals: the count first, then the first offending edge */
    const double good[4] = { 0.0, 100.0, 1000.0, 1e6 };
    CHECK(spectrum_edges_check(good, 4, &bad) == SPECTRUM_OK && bad == -1);
    CHECK(spectrum_edges_check(good, 2, &bad) == SPECTRUM_OK);
    CHECK(spectrum_edges_check(good, 1, &bad) == SPECTRUM_COUNT && bad == -1);
    CHECK(spectrum_edges_check(good, 0, &bad) == SPECTRUM_COUNT);
    CHECK(spectrum_edges_check(good, -3, &bad) == SPECTRUM_COUNT);
    CHECK(spectrum_edges_check(nullptr, 4, &bad) == SPECTRUM_NULL);
    CHECK(spectrum_edges_check(nullptr, 34, &bad) == SPECTRUM_COUNT);
    const double desc[3] = { 10.0, 20.0, 15.0 }, same[3] = { 10.0, 10.0, 20.0 }, neg[2] = { -1.0, 5.0 }, has_nan[3] = { 1.0, nan, 3.0 }, has_inf[2] = { 1.0, inf },
                 minus_zero[2] = { -0.0, 1.0 };
    CHECK(spectrum_edges_check(desc, 3, &bad) == SPECTRUM_ORDER && bad == 2);
    CHECK(spectrum_edges_check(same, 3, &bad) == SPECTRUM_ORDER && bad == 1);
    CHECK(spectrum_edges_check(neg, 2, &bad) == SPECTRUM_VALUE && bad == 0);
    CHECK(spectrum_edges_check(has_nan, 3, &bad) == SPECTRUM_VALUE && bad == 1);
    CHECK(spectrum_edges_check(has_inf, 2, &bad) == SPECTRUM_VALUE && bad == 1);
    CHECK(spectrum_edges_check(minus_zero, 2, &bad) == SPECTRUM_OK);
    std::vector<double> many(34);
    for (int i = 0; i < 34; i++) many[(size_t)i] = (double)i;
    CHECK(spectrum_edges_check(many.data(), 33, &bad) == SPECTRUM_OK);
    CHECK(spectrum_edges_check(many.data(), 34, &bad) == SPECTRUM_COUNT);
    /* the bins: on a bin, above Nyquist, values no integer type holds */
    CHECK(spectrum_k_lo(0.0, 48000) == 0 && spectrum_k_lo(-0.0, 48000) == 0);
    CHECK(spectrum_k_lo(24000.0, 48000) == 4096 && spectrum_k_lo(24000.1, 48000) == 4097 && spectrum_k_lo(1e300, 48000) == 4097);
    CHECK(spectrum_k_lo(1.7976931348623157e308, 1) == 4097);             /* the product overflows to +inf: clamped, never converted */
    CHECK(spectrum_k_lo(100.0 * 48000.0 / 8192.0, 48000) == 100);
    const gdg_spectrum_bands b = spectrum_bands(many.data(), 33, 8192);     /* 1 Hz per bin */
    CHECK(b.n_bands == 32);
    for (int i = 0; i < 33; i++) CHECK(b.k_lo[i] == i);
    const gdg_spectrum_bands two = spectrum_bands(good, 2, 48000);
    CHECK(two.n_bands == 1 && two.k_lo[0] == 0 && two.k_lo[1] == 18);       /* ceil(100 * 8192 / 48000) = ceil(17.07) */
    for (int i = 2; i < GDG_SPECTRUM_MAX_EDGES; i++) CHECK(two.k_lo[i] == GDG_SPECTRUM_BINS);
    if (failures) { printf("FAILED %d\n", failures); return 1; }
    printf("OK");
    const unsigned long rate = argc > 1 ? strtoul(argv[1], nullptr, 10) : 48000ul;
    for (int i = 2; i < argc; i++) printf(" %d", spectrum_k_lo(strtod(argv[i], nullptr), (uint32_t)rate));
    std::vector<double> w((size_t)GDG_SPECTRUM_BLOCK);
    spectrum_window(w.data());
    for (double v : w) printf(" %a", v);
    printf("\n");
    return 0;
}
