// import_driver.cpp — plays csrc/import_math.h on the host for tests/test_import_cpu.py: the header the import kernel includes,
// compiled stand-alone with the address and undefined-behaviour sanitizers and -ffp-contract=off, run as a child process.
// stdin: one request per line:
//   c is_ascii vertex_bytes off0 .. off61     (decimal) the checks of a caller's header             -> "c verdict property"
//   h vertex_bytes off0 .. off61              (decimal) the layout of the rows that follow            -> no answer
//   r <2 * vertex_bytes hexadecimal digits>   one row: fetched as words when the layout allows it, from bytes otherwise,
//   b <2 * vertex_bytes hexadecimal digits>   ... always from bytes;                                  -> "r" | "b" and the 56 words of the record
// Every row lives in a heap block of exactly vertex_bytes bytes: a fetch outside the row is a sanitizer report.
// stdout: one answer per request, in order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "import_math.h"

using namespace gsx;

static_assert(sizeof(gsx_gaussian) == 224, "a record is 56 words");
static_assert(sizeof(ImportLayout) == 4 + 4 * kImportProps, "the layout is a stride and 62 offsets");

static int hex_digit(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

int main() {
    char* line = nullptr;
    size_t cap = 0;
    ImportLayout lay{};
    bool have_layout = false;
    std::string out;
    while (getline(&line, &cap, stdin) > 0) {
        const char mode = line[0];
        if (mode == 'c' || mode == 'h') {
            long w[2 + kImportProps];
            const int need = mode == 'c' ? 2 + kImportProps : 1 + kImportProps;
            char* p = line + 1;
            int got = 0;
            for (; got < need; ++got) {
                char* end = nullptr;
                w[got] = strtol(p, &end, 10);
                if (end == p) break;
                p = end;
            }
            if (got != need) {
                fprintf(stderr, "bad request '%c' with %d numbers\n", mode, got);
                return 2;
            }
            gsx_ply_header h{};
            h.is_ascii = mode == 'c' ? (uint32_t)w[0] : 0u;
            h.vertex_bytes = (uint32_t)w[mode == 'c' ? 1 : 0];
            for (int k = 0; k < kImportProps; ++k) h.offsets[k] = (int32_t)w[need - kImportProps + k];
            int bad = -1;
            const int verdict = im_check_header(h, &bad);
            if (mode == 'c') {
                printf("c %d %d\n", verdict, bad);
            } else {
                if (verdict != 0) {
                    fprintf(stderr, "the layout fails the header checks (%d, property %d)\n", verdict, bad);
                    return 2;
                }
                lay = im_layout(h);
                have_layout = true;
            }
            continue;
        }
        if ((mode != 'r' && mode != 'b') || !have_layout) {
            fprintf(stderr, "bad request '%c'\n", mode);
            return 2;
        }
        const char* p = line + 1;
        while (*p == ' ') ++p;
        uint8_t* row = static_cast<uint8_t*>(malloc(lay.stride));  // exactly the row (malloc: aligned for words)
        for (uint32_t k = 0; k < lay.stride; ++k) {
            const int hi = hex_digit(p[2 * k]), lo = hi < 0 ? -1 : hex_digit(p[2 * k + 1]);
            if (lo < 0) {
                fprintf(stderr, "a row of %u bytes needs %u hexadecimal digits\n", lay.stride, 2 * lay.stride);
                free(row);
                return 2;
            }
            row[k] = (uint8_t)(hi << 4 | lo);
        }
        float v[kImportProps];
        if (mode == 'r' && im_is_word_aligned(lay)) im_fetch_words(reinterpret_cast<const uint32_t*>(row), lay, v);
        else im_fetch_bytes(row, lay, v);
        free(row);
        gsx_gaussian g;
        im_row_to_gaussian(v, &g);
        uint32_t words[56];
        memcpy(words, &g, sizeof g);
        out.assign(1, mode);
        char buf[16];
        for (int k = 0; k < 56; ++k) {
            snprintf(buf, sizeof buf, " %x", words[k]);
            out += buf;
        }
        puts(out.c_str());
    }
    free(line);
    return 0;
}
