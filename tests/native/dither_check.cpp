/* csrc/dither.h on the host, under AddressSanitizer and UBSan (tests/test_dither_host.py): the hash, the key, the noise and the quantiser
 * against the known answers of include/gdg.h and against a table the Python side made with its numpy restatement; the row-to-port
 * mapping, the range check of port_base + n and the master cursor's overflow.  No device, no context.
 * Usage: dither_check [table]   -- a line of the table: seed port index x-bits h code8 code16 code24 code32 (hex, hex, hex, hex, hex, 4 decimals) */
#include "dither.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static long long code_of(int fmt, double x, uint64_t seed, uint32_t port, uint64_t index) {
    return gdg_dither_quantise(fmt, x, gdg_dither_noise(gdg_dither_hash(gdg_dither_key(seed, port), index)));
}

/* the signed code back from the little-endian bytes gdg_dither_code returns */
static long long signed_of(int fmt, unsigned code) {
    if (fmt == 0) return (long long)code - 128;
    const int bits = fmt == 1 ? 16 : fmt == 2 ? 24 : 32;
    long long v = (long long)code;
    if (v >= (1ll << (bits - 1))) v -= (1ll << bits);
    return v;
}

struct Known { uint64_t seed; uint32_t port; uint64_t index; double x; uint64_t h; long long c16, c24; };

int main(int argc, char **argv) {
    const Known known[7] = {
        { 0x0ull, 0u, 0ull, 0.0, 0xdf9545e13007448aull, 1, 1 },
        { 0x1ull, 0u, 0ull, 0.25, 0x8dde58528d955053ull, 8192, 2097152 },
        { 0x3039ull, 7u, 0xffffffffull, 0.25, 0xebb51d375a797963ull, 8192, 2097152 },
        { 0x3039ull, 7u, 0x100000000ull, -0.7, 0xe8f8277b0aa97796ull, -22936, -5872024 },
        { 0xdeadbeefcafef00dull, 0xfffffffdu, (1ull << 40) + 1, 1.5, 0x71a1a79a27a98aecull, 32767, 8388607 },
        { 0x63ull, 3u, 8191ull, -1.0, 0xaedc319de87b0798ull, -32768, -8388608 },
        { 0x63ull, 3u, 8192ull, 1e-5, 0x33a34e84d34b5c4bull, 0, 83 },
    };
    for (const Known &k : known) {
        CHECK(gdg_dither_hash(gdg_dither_key(k.seed, k.port), k.index) == k.h);
        CHECK(code_of(1, k.x, k.seed, k.port, k.index) == k.c16);
        CHECK(code_of(2, k.x, k.seed, k.port, k.index) == k.c24);
        for (int fmt = 0; fmt < 4; fmt++)
            CHECK(signed_of(fmt, gdg_dither_code(fmt, k.x, gdg_dither_key(k.seed, k.port), k.index)) == code_of(fmt, k.x, k.seed, k.port, k.index));
    }
    /* the noise: triangular on (-1, 1), its two ends */
    CHECK(gdg_dither_noise(0xffffffff00000000ull) == 4294967295.0 / 4294967296.0);
    CHECK(gdg_dither_noise(0x00000000ffffffffull) == -4294967295.0 / 4294967296.0);
    CHECK(gdg_dither_noise(0x1234567812345678ull) == 0.0);
    /* full scale never wraps, whatever the noise */
    for (int fmt = 0; fmt < 4; fmt++) {
        const double hi = fmt == 0 ? 127.0 : fmt == 1 ? 32767.0 : fmt == 2 ? 8388607.0 : 2147483647.0;
        CHECK(gdg_dither_quantise(fmt, 7.5, 0.999) == (long long)hi && gdg_dither_quantise(fmt, -7.5, -0.999) == -(long long)hi - 1);
    }
    /* which dither applies: mode 1 on an LPCM format */
    for (int fmt = -1; fmt < 8; fmt++) {
        CHECK(!gdg_dither_applies(0, fmt) && !gdg_dither_applies(2, fmt));
        CHECK(gdg_dither_applies(1, fmt) == (fmt >= 0 && fmt <= 3));
    }
    /* rows -> ports: chain rows from port_base, then master left, master right, metronome */
    CHECK(gdg_dither_row_port(0, 4, 0) == 0 && gdg_dither_row_port(0, 4, 3) == 3);
    CHECK(gdg_dither_row_port(0, 4, 4) == 0xfffffffdu && gdg_dither_row_port(0, 4, 5) == 0xfffffffeu && gdg_dither_row_port(0, 4, 6) == 0xffffffffu);
    CHECK(gdg_dither_row_port(1000, 2, 1) == 1001 && gdg_dither_row_port(1000, 2, 2) == 0xfffffffdu);
    CHECK(gdg_dither_row_port(0xfffffffcu - 1, 2, 1) == 0xfffffffcu);
    CHECK(gdg_dither_row_port(GDG_DITHER_PORT_METRONOME, 1, 0) == 0xffffffffu);      /* a shard's metronome track on its own */
    CHECK(gdg_dither_row_port(0, 0, 0) == GDG_DITHER_PORT_MASTER_LEFT && gdg_dither_row_port(0, 0, 1) == GDG_DITHER_PORT_MASTER_RIGHT);
    /* port_base + n stays below the fixed ids */
    CHECK(gdg_dither_ports_ok(0, 0) && gdg_dither_ports_ok(0, 512) && gdg_dither_ports_ok(0xfffffffcu, 0) && gdg_dither_ports_ok(0xfffffffbu, 1));
    CHECK(!gdg_dither_ports_ok(0xfffffffcu, 1) && !gdg_dither_ports_ok(0xfffffffdu, 0) && !gdg_dither_ports_ok(0xffffffffu, 1));
    CHECK(gdg_dither_ports_ok(0xfffffffdu - 512u - 1u, 512) && !gdg_dither_ports_ok(0xfffffffdu - 512u, 512) && !gdg_dither_ports_ok(0, -1));
    CHECK(gdg_dither_ports_ok(0x80000000u, 0x7fffffff - 3) && !gdg_dither_ports_ok(0x80000000u, 0x7fffffff));
    /* the cursor */
    uint64_t next = 7;
    CHECK(gdg_dither_advance(0, 8192, &next) && next == 8192);
    CHECK(gdg_dither_advance(~(uint64_t)0 - 8192, 8192, &next) && next == ~(uint64_t)0);
    next = 7;
    CHECK(!gdg_dither_advance(~(uint64_t)0 - 8191, 8192, &next) && next == 7);
    CHECK(gdg_dither_advance(~(uint64_t)0, 0, &next) && next == ~(uint64_t)0);

    long rows = 0;
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
        uint64_t seed, port, index, xbits, h;
        long long want[4];
        while (fscanf(f, "%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %lld %lld %lld %lld", &seed, &port, &index, &xbits, &h,
                      &want[0], &want[1], &want[2], &want[3]) == 9) {
            double x;
            memcpy(&x, &xbits, sizeof x);
            const uint64_t key = gdg_dither_key(seed, (uint32_t)port);
            const int before = failures;
            CHECK(gdg_dither_hash(key, index) == h);
            for (int fmt = 0; fmt < 4; fmt++) {
                CHECK(code_of(fmt, x, seed, (uint32_t)port, index) == want[fmt]);
                CHECK(signed_of(fmt, gdg_dither_code(fmt, x, key, index)) == want[fmt]);
            }
            if (failures != before && failures < 20)
                fprintf(stderr, "  row %ld: seed %" PRIx64 " port %" PRIx64 " index %" PRIx64 " x %.17g\n", rows, seed, port, index, x);
            rows++;
        }
        fclose(f);
    }
    if (failures) { printf("FAILED: %d checks\n", failures); return 1; }
    printf("OK %ld rows\n", rows);
    return 0;
}
