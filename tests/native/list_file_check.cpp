/*
 * list_file_check.cpp -- the host stores of the list records without HIP: a step's section of [rows][w] elements that has come down is filed
 * into a store of [rows][blocks] under the blocks from b0 on (csrc/report_sections.h: list_file_rows, the copy rule under ctx.h's
 * list_file).  Every byte has to land where the formulas it replaced put it -- the fits' (per fit f: store[(f * blocks + b0) * 368 ..] from
 * section[f * w * 368 ..], w * 368 bytes) and, with one row, the Gram's and the tap fits' (store[b0 * rec ..] from section[0 ..], w * rec
 * bytes), spelled out here -- and nothing else may be written.  Built by tests/test_list_records_host.py, once more under
 * AddressSanitizer and UBSan: the vectors are exactly as long as the store and the section, so a byte past either is reported.
 */
#include "report_sections.h"

#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

int main() {
    const size_t blocks = 3;
    int cases = 0;
    for (size_t rows : { (size_t)1, (size_t)3 })
        for (size_t w : { (size_t)1, (size_t)2 })
            for (size_t elem : { (size_t)FIT_RECORD_BYTES, gram_record_bytes(3), (size_t)10 * 8 })
                for (size_t b0 = 0; b0 + w <= blocks; b0++) {
                    const unsigned char untouched = 0xA5;
                    std::vector<unsigned char> store(rows * blocks * elem, untouched), want(store), section(rows * w * elem);
                    for (size_t i = 0; i < section.size(); i++) section[i] = (unsigned char)(1 + i % 151);      /* never 0xA5: 1 .. 151 */
                    /* the old formulas, by hand */
                    if (rows == 1) memcpy(want.data() + b0 * elem, section.data(), w * elem);                  /* gram_file, tapfit_file */
                    else for (size_t f = 0; f < rows; f++) memcpy(&want[(f * blocks + b0) * elem], section.data() + f * w * elem, w * elem);      /* fit_file */
                    list_file_rows(store.data(), blocks, { rows, elem }, section.data(), w, b0);
                    CHECK(store == want);
                    /* ... and said once more without a copy: element (r, b) of the store is element (r, b - b0) of the section or untouched */
                    for (size_t r = 0; r < rows; r++)
                        for (size_t b = 0; b < blocks; b++)
                            for (size_t i = 0; i < elem; i++) {
                                const unsigned char got = store[(r * blocks + b) * elem + i];
                                const bool filed = b >= b0 && b < b0 + w;
                                if (got != (filed ? section[(r * w + (b - b0)) * elem + i] : untouched)) { CHECK(!"a byte is not where it belongs"); r = rows; b = blocks; break; }
                            }
                    cases++;
                }
    /* a list that is off has no rows to file: nothing is read or written */
    list_file_rows(nullptr, blocks, { 0, 0 }, nullptr, 2, 0);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("OK list stores; %d cases\n", cases);
    return 0;
}
