/*
 * list_chain_check.cpp -- the one chain of the five list records (csrc/report_sections.h) against the rule it replaced, without HIP.  THE OLD
 * RULE, restated here as formulas: the three kinds' sections chained behind `base`, then the transfer records' section behind their end, then
 * the delivered rows' records' behind that; each section starts at (end + 15) & ~15 and holds rows * w * elem bytes, or takes no byte when its
 * kind is off.  Over all 32 on/off masks of the five kinds, w = 1, 2, 3, 4, 16 and base = 0, 8, 40, 4096, with 2 fits, a Gram list of 3 ports,
 * tap fits of 21 doubles, 2 transfer pairs in groups of 32 and the delivered rows' records of 5 ports: list_sections puts every section where
 * the old rule did, lists_room is the sum of the 16 + rows * W * elem of the kinds that are on, a step of the whole window fits that room, and
 * some section's end lies off a 16-byte boundary, so that the next one is moved.  Built by tests/test_list_records_host.py.
 */
#include "report_sections.h"

#include <cstdio>
#include <initializer_list>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

int main() {
    static_assert(LIST_FIT == 0 && LIST_GRAM == 1 && LIST_TAPFIT == 2 && LIST_TRANSFER == 3 && LIST_DELIVERED == 4 && LIST_KINDS == 5, "the sections ride in this order");
    const size_t rows[5] = { 2, 1, 1, 1, 5 }, elem[5] = { 368, 3 * 4 / 2 * 8, 21 * 8, 2 * (4096 / 32 + 1) * 4 * 8, 40 };
    CHECK(FIT_RECORD_BYTES == elem[0] && gram_record_bytes(3) == elem[1] && transfer_record_bytes(2, 32) == elem[3] && DELIVERED_RECORD_BYTES == elem[4]);
    int cases = 0, ends_off = 0, ragged = 0, moved = 0;
    for (int mask = 0; mask < 32; mask++)
        for (size_t w : { (size_t)1, (size_t)2, (size_t)3, (size_t)4, (size_t)16 })
            for (size_t base : { (size_t)0, (size_t)8, (size_t)40, (size_t)4096 }) {
                ListShape shape[LIST_KINDS];
                for (int k = 0; k < 5; k++) shape[k] = { rows[k], (mask >> k) & 1 ? elem[k] : 0 };
                const ListSections got = list_sections(base, shape, w);
                /* the old rule: three chained sections ... */
                size_t at[5], bytes[5], end = base, room = 0;
                for (int k = 0; k < 3; k++) {
                    const bool on = (mask >> k) & 1;
                    at[k] = on ? up16(end) : end;
                    bytes[k] = on ? rows[k] * w * elem[k] : 0;
                    end = at[k] + bytes[k];
                }
                const size_t three_end = end;
                /* ... then the transfer records behind their end ... */
                at[3] = (mask & 8) ? up16(three_end) : three_end;
                bytes[3] = (mask & 8) ? 1 * w * elem[3] : 0;
                const size_t transfer_end = at[3] + bytes[3];
                /* ... then the delivered rows' records behind that */
                at[4] = (mask & 16) ? up16(transfer_end) : transfer_end;
                bytes[4] = (mask & 16) ? 5 * w * 40 : 0;
                const size_t delivered_end = at[4] + bytes[4];
                for (int k = 0; k < 5; k++) {
                    CHECK(got.of[k].at == at[k] && got.of[k].bytes == bytes[k] && got.of[k].end == at[k] + bytes[k]);
                    if ((mask >> k) & 1) {
                        CHECK(got.of[k].at % 16 == 0);
                        if (got.of[k].end % 16) ends_off++;                      /* the delivered rows' 40 * 5 * w at odd w */
                        room += 16 + rows[k] * w * elem[k];
                        const size_t before = k ? at[k - 1] + bytes[k - 1] : base;
                        if (before % 16) ragged++;
                        if (got.of[k].at != before) moved++;
                    }
                }
                CHECK(got.end == delivered_end);
                CHECK(lists_room(shape, w) == room && got.end - base <= room);
                if (!mask) CHECK(got.end == base && room == 0);
                cases++;
            }
    CHECK(ends_off > 0 && ragged > 0 && moved == ragged);                                       /* base = 8 and 40 * 5 * 1 both end off a boundary: the alignment path ran */
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("OK one chain; %d cases, %d sections behind an end off a 16-byte boundary\n", cases, ragged);
    return 0;
}
