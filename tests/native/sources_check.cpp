/* csrc/batch_sources.h on the host, under AddressSanitizer and UBSan (tests/test_batch_sources_host.py): the validation of a source map,
 * readers -> roots, and per root the list of rows it feeds, over hand-written maps and seeded random ones.  No device, no context. */
#include "batch_sources.h"
#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static unsigned long long lcg(unsigned long long &s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

/* the rows of a root from the fans against the definition, and every channel in exactly one list */
static void check_fans(const std::vector<int> &map) {
    const int n = (int)map.size();
    const SourceFans fans = sources_fans(map);
    CHECK((int)fans.first.size() == n + 1 && fans.first[0] == 0);
    std::vector<int> seen((size_t)n, 0);
    int readers = 0;
    for (int r = 0; r < n; r++) {
        if (map[(size_t)r] != r) { CHECK(fans.fan(r) == 0); continue; }
        seen[(size_t)r]++;
        int last = -1;
        for (int k = 0; k < fans.fan(r); k++) {
            const int c = fans.readers(r)[k];
            CHECK(c >= 0 && c < n && c != r && map[(size_t)c] == r && c > last);
            CHECK(sources_root(map, c) == r);
            last = c;
            seen[(size_t)c]++;
            readers++;
        }
    }
    for (int c = 0; c < n; c++) CHECK(seen[(size_t)c] == 1);
    CHECK((int)fans.list.size() == readers);
    CHECK(sources_have_reader(map) == (readers > 0));
}

int main(int argc, char **argv) {
    unsigned long long seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 2000;
    int bad = 0;
    /* the issue's map and its refusals */
    const int core[6] = { 0, 0, 2, 0, 2, 5 };
    CHECK(sources_check(core, 6, 6, &bad) == SOURCES_OK && bad == -1);
    check_fans(std::vector<int>(core, core + 6));
    const SourceFans f = sources_fans(std::vector<int>(core, core + 6));
    CHECK(f.fan(0) == 2 && f.readers(0)[0] == 1 && f.readers(0)[1] == 3 && f.fan(2) == 1 && f.readers(2)[0] == 4 && f.fan(5) == 0);
    CHECK(sources_check(core, 5, 6, &bad) == SOURCES_WRONG_N);
    CHECK(sources_check(core, 6, 7, &bad) == SOURCES_WRONG_N);
    CHECK(sources_check(nullptr, 6, 6, &bad) == SOURCES_WRONG_N);
    const int high[6] = { 0, 0, 2, 0, 6, 5 }, low[6] = { 0, 0, 2, -1, 2, 5 }, chain[6] = { 0, 0, 1, 0, 2, 5 }, loop[2] = { 1, 0 };
    CHECK(sources_check(high, 6, 6, &bad) == SOURCES_OUT_OF_RANGE && bad == 4);
    CHECK(sources_check(low, 6, 6, &bad) == SOURCES_OUT_OF_RANGE && bad == 3);
    CHECK(sources_check(chain, 6, 6, &bad) == SOURCES_CHAIN && bad == 2);
    CHECK(sources_check(loop, 2, 2, &bad) == SOURCES_CHAIN && bad == 0);
    CHECK(!sources_have_reader(std::vector<int>()) && sources_root(std::vector<int>(), 3) == 3);
    check_fans(std::vector<int>());
    /* random maps: valid ones by construction, then one entry spoilt */
    for (int round = 0; round < rounds; round++) {
        const int n = 1 + (int)(lcg(seed) % 600);
        std::vector<int> roots, map((size_t)n);
        for (int c = 0; c < n; c++) if (c == 0 || lcg(seed) % 8 == 0) roots.push_back(c);
        std::vector<char> is_root((size_t)n, 0);
        for (int r : roots) is_root[(size_t)r] = 1;
        for (int c = 0; c < n; c++) map[(size_t)c] = is_root[(size_t)c] ? c : roots[lcg(seed) % roots.size()];
        CHECK(sources_check(map.data(), n, n, &bad) == SOURCES_OK);
        check_fans(map);
        std::vector<int> spoilt(map);
        const int at = (int)(lcg(seed) % (unsigned)n);
        switch (lcg(seed) % 3) {
        case 0: spoilt[(size_t)at] = n + (int)(lcg(seed) % 5); CHECK(sources_check(spoilt.data(), n, n, &bad) == SOURCES_OUT_OF_RANGE && bad == at); break;
        case 1: spoilt[(size_t)at] = -1 - (int)(lcg(seed) % 5); CHECK(sources_check(spoilt.data(), n, n, &bad) == SOURCES_OUT_OF_RANGE && bad == at); break;
        default: {
            /* a reader made to read another reader, where there are two */
            int r1 = -1, r2 = -1;
            for (int c = 0; c < n; c++) if (!is_root[(size_t)c]) { if (r1 < 0) r1 = c; else { r2 = c; break; } }
            if (r2 < 0) break;
            spoilt = map;
            spoilt[(size_t)r2] = r1;
            CHECK(sources_check(spoilt.data(), n, n, &bad) == SOURCES_CHAIN && bad == r2);
        }
        }
    }
    if (failures) { printf("FAILED %d checks\n", failures); return 1; }
    printf("OK %d rounds\n", rounds);
    return 0;
}
