/* csrc/align_map.h on the host, under AddressSanitizer and UBSan (tests/test_align_host.py): the validation of a reference list, the rule by
 * which a list replaces the one in force, and the list cut into launches.  No device, no context.
 *   align_check MAX_LAG REF...   "OK", then "port:ref" for every measured port in launch order, a "|" between two launches */
#include "align_map.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

int main(int argc, char **argv) {
    int bad = 0;
    /* good lists: every port against port 0, itself included; nothing measured; a chain of references */
    const int star[5] = { 0, 0, 0, 0, 0 }, none[3] = { -1, -1, -1 }, chain[4] = { -1, 0, 1, 2 }, self[1] = { 0 };
    CHECK(align_map_check(star, 5, 2048, &bad) == ALIGN_OK && bad == -1);
    CHECK(align_map_check(none, 3, 1, &bad) == ALIGN_OK);
    CHECK(align_map_check(chain, 4, 64, &bad) == ALIGN_OK);
    CHECK(align_map_check(self, 1, 1, &bad) == ALIGN_OK);
    /* out-of-range references: the first offender is named */
    const int past[4] = { 0, 4, 0, 7 }, below[3] = { 0, 0, -2 }, short_list[2] = { 0, 1 };
    CHECK(align_map_check(past, 4, 64, &bad) == ALIGN_REF && bad == 1);
    CHECK(align_map_check(below, 3, 64, &bad) == ALIGN_REF && bad == 2);
    CHECK(align_map_check(short_list, 2, 64, &bad) == ALIGN_OK);
    CHECK(align_map_check(short_list, 1, 64, &bad) == ALIGN_OK);             /* one port: entry 1 is not looked at */
    /* the lag range */
    CHECK(align_map_check(star, 5, 0, &bad) == ALIGN_LAG && bad == -1);
    CHECK(align_map_check(star, 5, 2049, &bad) == ALIGN_LAG);
    CHECK(align_map_check(star, 5, -1, &bad) == ALIGN_LAG);
    CHECK(align_map_check(star, 5, 1, &bad) == ALIGN_OK && align_map_check(star, 5, 2048, &bad) == ALIGN_OK);
    /* an empty list, no list */
    CHECK(align_map_check(star, 0, 64, &bad) == ALIGN_COUNT);
    CHECK(align_map_check(star, -2, 64, &bad) == ALIGN_COUNT);
    CHECK(align_map_check(nullptr, 3, 64, &bad) == ALIGN_NULL);
    CHECK(align_map_check(nullptr, 0, 64, &bad) == ALIGN_COUNT);
    /* a list replaces the one in force only when it is valid as a whole */
    std::vector<int> map;
    int lag = 0;
    CHECK(align_map_replace(map, lag, chain, 4, 64, &bad) == ALIGN_OK && map.size() == 4 && map[3] == 2 && lag == 64);
    CHECK(align_map_replace(map, lag, past, 4, 100, &bad) == ALIGN_REF && bad == 1 && map.size() == 4 && map[1] == 0 && map[3] == 2 && lag == 64);
    CHECK(align_map_replace(map, lag, star, 5, 4000, &bad) == ALIGN_LAG && map.size() == 4 && lag == 64);
    CHECK(align_map_replace(map, lag, nullptr, 5, 64, &bad) == ALIGN_NULL && map.size() == 4);
    CHECK(align_map_replace(map, lag, star, 5, 2048, &bad) == ALIGN_OK && map.size() == 5 && lag == 2048);
    /* the launches: measured ports in ascending order, 240 to a piece; a skipped port neither measured nor referenced */
    CHECK(align_map_pieces(std::vector<int>(none, none + 3), 64).empty());
    std::vector<gdg_align_pairs> one = align_map_pieces(std::vector<int>(chain, chain + 4), 64);
    CHECK(one.size() == 1 && one[0].n == 3 && one[0].max_lag == 64 && one[0].port[0] == 1 && one[0].ref[0] == 0 && one[0].port[2] == 3 && one[0].ref[2] == 2);
    one = align_map_pieces(std::vector<int>(chain, chain + 4), 64, 2);        /* port 2 out: 2 itself and 3, which references it */
    CHECK(one.size() == 1 && one[0].n == 1 && one[0].port[0] == 1);
    std::vector<int> many(515, 0);
    many[7] = -1;
    std::vector<gdg_align_pairs> cut = align_map_pieces(many, 2048);
    CHECK(cut.size() == 3 && cut[0].n == GDG_ALIGN_PAIRS && cut[1].n == GDG_ALIGN_PAIRS && cut[2].n == 514 - 2 * GDG_ALIGN_PAIRS);
    CHECK(cut[0].port[7] == 8 && cut[1].port[0] == GDG_ALIGN_PAIRS + 1 && cut[2].port[cut[2].n - 1] == 514);
    if (failures) { printf("FAILED %d\n", failures); return 1; }
    printf("OK");
    if (argc > 2) {
        const int max_lag = atoi(argv[1]);
        std::vector<int> ref;
        for (int i = 2; i < argc; i++) ref.push_back(atoi(argv[i]));
        const int st = align_map_check(ref.data(), (int)ref.size(), max_lag, &bad);
        printf(" %d %d", st, bad);
        if (st == ALIGN_OK) {
            const std::vector<gdg_align_pairs> pieces = align_map_pieces(ref, max_lag);
            for (size_t k = 0; k < pieces.size(); k++) {
                if (k) printf(" |");
                for (int i = 0; i < pieces[k].n; i++) printf(" %d:%d", pieces[k].port[i], pieces[k].ref[i]);
            }
        }
    }
    printf("\n");
    return 0;
}
