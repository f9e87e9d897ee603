// property_driver.cpp — csrc/property_math.h (the values, bins, hit test and selection op of the model properties, spec §17) played
// on the host, for tests/test_property_cpu.py: a stand-alone program the test builds with the address and undefined-behaviour
// sanitizers and -ffp-contract=off.  Every float crosses as the hex of its bits.  stdin, one command a line:
//   "xform <9 R> <3 s> <3 t>"            the transform of the "pc" commands that follow (default: identity values)
//   "pc <property> <world> <x y z colour> ..."   stdout "values <hex> ..."   : prop_value_pc of every element
//   "scale <property> <6 words> ..."      stdout "values <hex> ..."           : prop_value_scale of every covariance
//   "range <lo> <hi> <bins>"              stdout "live <0|1>", "edges <hex x (bins + 1)>"; sets the range of what follows
//   "classify <v> ..."                    stdout "class <bin | -1 non-finite | -2 below | -3 above> ..."
//   "hit <use_bins> <bin_lo> <bin_hi> <v> ..."   stdout "hit <0|1> ..."
//   "minmax <v> ..."                      stdout "minmax <count> <min hex> <max hex>" over the finite values, by prop_key
//   "op <op> <n> <old words> | <hit words>"      stdout "new <hex words>" : prop_apply_op, tail bits cleared
//   "sweep"                               every float32 of [lo, hi] in order: stdout "sweep <values> <violations>", a violation being
//                                         a bin whose edges do not enclose the value, a bin below the one before, or a bin >= bins
//                                         (a range that is not live: a bin other than 0)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "extract_math.h"
#include "property_math.h"

using namespace gsx;

static std::vector<uint32_t> words(const char* s) {
    std::vector<uint32_t> v;
    char* end = nullptr;
    for (;;) {
        while (*s == ' ' || *s == '|') ++s;
        const unsigned long x = strtoul(s, &end, 16);
        if (end == s) break;
        v.push_back((uint32_t)x);
        s = end;
    }
    return v;
}
static void print_words(const char* tag, const std::vector<uint32_t>& v) {
    printf("%s", tag);
    for (uint32_t w : v) printf(" %x", w);
    printf("\n");
}

int main() {
    PropTransform xf = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {1, 1, 1}, {0, 0, 0}};
    PropRange range = prop_range(0.0f, 1.0f, 1u);
    std::string line;
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        line = buf;
        while (!line.empty() && line.back() != '\n' && fgets(buf, sizeof buf, stdin)) line += buf;
        const char* s = line.c_str();
        char cmd[32] = {0};
        int used = 0;
        if (sscanf(s, "%31s%n", cmd, &used) != 1) continue;
        s += used;
        if (!strcmp(cmd, "xform")) {
            const std::vector<uint32_t> w = words(s);
            if (w.size() != 15) return 2;
            for (int k = 0; k < 9; ++k) xf.R[k] = prop_from_bits(w[k]);
            for (int k = 0; k < 3; ++k) {
                xf.s[k] = prop_from_bits(w[9 + k]);
                xf.t[k] = prop_from_bits(w[12 + k]);
            }
        } else if (!strcmp(cmd, "pc")) {
            unsigned property = 0, world = 0;
            if (sscanf(s, "%u %u%n", &property, &world, &used) != 2) return 2;
            const std::vector<uint32_t> w = words(s + used);
            if (w.size() % 4) return 2;
            std::vector<uint32_t> out;
            for (size_t i = 0; i < w.size(); i += 4) out.push_back(ex_bits(prop_value_pc(property, w[i], w[i + 1], w[i + 2], w[i + 3], world != 0, xf)));
            print_words("values", out);
        } else if (!strcmp(cmd, "scale")) {
            unsigned property = 0;
            if (sscanf(s, "%u%n", &property, &used) != 1) return 2;
            const std::vector<uint32_t> w = words(s + used);
            if (w.size() % 6) return 2;
            std::vector<uint32_t> out;
            for (size_t i = 0; i < w.size(); i += 6) {
                float c[6];
                for (int k = 0; k < 6; ++k) c[k] = prop_from_bits(w[i + k]);
                out.push_back(ex_bits(prop_value_scale(property, c)));
            }
            print_words("values", out);
        } else if (!strcmp(cmd, "range")) {
            unsigned lo = 0, hi = 0, bins = 0;
            if (sscanf(s, "%x %x %u", &lo, &hi, &bins) != 3) return 2;
            range = prop_range(prop_from_bits(lo), prop_from_bits(hi), bins);
            printf("live %d\n", range.live ? 1 : 0);
            std::vector<uint32_t> e;
            for (uint32_t b = 0; b <= range.bins; ++b) e.push_back(ex_bits(prop_edge(range, b)));
            print_words("edges", e);
        } else if (!strcmp(cmd, "classify")) {
            printf("class");
            for (uint32_t w : words(s)) {
                const uint32_t c = prop_classify(range, prop_from_bits(w));
                printf(" %d", c == kPropNonfinite ? -1 : (c == kPropBelow ? -2 : (c == kPropAbove ? -3 : (int)c)));
            }
            printf("\n");
        } else if (!strcmp(cmd, "hit")) {
            unsigned use_bins = 0, bin_lo = 0, bin_hi = 0;
            if (sscanf(s, "%u %u %u%n", &use_bins, &bin_lo, &bin_hi, &used) != 3) return 2;
            printf("hit");
            for (uint32_t w : words(s + used)) printf(" %d", prop_hit(range, prop_from_bits(w), use_bins != 0, bin_lo, bin_hi) ? 1 : 0);
            printf("\n");
        } else if (!strcmp(cmd, "minmax")) {
            uint32_t mn = kPropKeyMinIdentity, mx = kPropKeyMaxIdentity, count = 0;
            for (uint32_t w : words(s)) {
                const float v = prop_from_bits(w);
                if (!prop_finite(v)) continue;
                ++count;
                mn = prop_key(v) < mn ? prop_key(v) : mn;
                mx = prop_key(v) > mx ? prop_key(v) : mx;
            }
            printf("minmax %u %x %x\n", count, count ? ex_bits(prop_unkey(mn)) : 0u, count ? ex_bits(prop_unkey(mx)) : 0u);
        } else if (!strcmp(cmd, "op")) {
            unsigned op = 0;
            unsigned long long n = 0;
            if (sscanf(s, "%u %llu%n", &op, &n, &used) != 2) return 2;
            const std::vector<uint32_t> w = words(s + used);
            const size_t nw = (size_t)((n + 31) / 32);
            if (w.size() != 2 * nw) return 2;
            std::vector<uint32_t> out(nw);
            for (size_t k = 0; k < nw; ++k) out[k] = prop_apply_op(op, w[k], w[nw + k]) & extract_tail_mask(n, k);
            print_words("new", out);
        } else if (!strcmp(cmd, "sweep")) {
            unsigned long long values = 0, violations = 0;
            uint32_t before = 0;
            for (uint64_t k = prop_key(range.lo); k <= (uint64_t)prop_key(range.hi); ++k) {
                const float v = prop_unkey((uint32_t)k);
                const uint32_t b = prop_classify(range, v);
                // (-0 and +0 are two keys and one value: both are in range when either end is a zero)
                // (a range that is not live has no edges to lie between: bin 0)
                const bool ok = range.live ? (b < range.bins && prop_edge(range, b) <= v && v <= prop_edge(range, b + 1) && b >= before) : b == 0u;
                if (!ok) ++violations;
                before = b < range.bins ? b : before;
                ++values;
            }
            printf("sweep %llu %llu\n", values, violations);
        } else {
            return 2;
        }
    }
    return 0;
}
