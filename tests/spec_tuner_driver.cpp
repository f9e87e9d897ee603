// spec_tuner_driver.cpp — plays a scripted sequence of frames against the speculation tuner's rules (csrc/spec_tuner.h) on the CPU and
// prints what they decided, one line per frame (tests/test_spec_tuner_cpu.py compiles and runs it).  Commands, one per line on stdin:
//   times S P       a speculated frame times S ms, a plain one P ms (default 1 1)
//   lanes L         frames in flight, for the "windows" column (default 1)
//   frames N MODE   N frames; what becomes of a bracketed frame's timing:  deliver  before the next frame's decision
//                                                                           withhold until the rules say the host must wait (or `flush`)
//                                                                           open     the bracket stays open (a later `drop` ends it)
//   flush           every withheld timing arrives
//   drop            the open bracket goes away without a timing
//   reset           SpecTunerRules::reset(); withheld timings are stale and discarded (the shell's job in the library)
//   state           prints  state len_spec len_plain n_spec n_plain probe_pending left
// Per frame:  frame_no phase speculates bracketed probe must_wait windows
//   must_wait: the rules asked for the probe's timings before this frame's decision (the withheld ones were then delivered)
//   windows:   this frame must leave windows behind for the next
#include <cstdio>
#include <cstring>
#include <vector>

#include "spec_tuner.h"

int main() {
    static const char* const names[] = {"SPEC", "PROBE_PLAIN", "SETTLE_SPEC", "PLAIN", "PROBE_SPEC", "SETTLE_PLAIN"};
    struct Timing { bool spec, probe; float ms; };
    gsx::SpecTunerRules t;
    std::vector<Timing> withheld;
    Timing open{};
    bool have_open = false;
    float ms_spec = 1.0f, ms_plain = 1.0f;
    unsigned lanes = 1;
    auto flush = [&withheld, &t]() {
        for (const Timing& w : withheld) t.timing(w.spec, w.probe, w.ms);
        withheld.clear();
    };
    char line[256], cmd[32], mode[32];
    while (fgets(line, sizeof line, stdin)) {
        unsigned n = 0;
        if (sscanf(line, "%31s", cmd) != 1) continue;
        if (!strcmp(cmd, "times") && sscanf(line, "%*s %f %f", &ms_spec, &ms_plain) == 2) continue;
        if (!strcmp(cmd, "lanes") && sscanf(line, "%*s %u", &lanes) == 1) continue;
        if (!strcmp(cmd, "flush")) { flush(); continue; }
        if (!strcmp(cmd, "drop")) {
            if (have_open && open.probe) t.probe_dropped();
            have_open = false;
            continue;
        }
        if (!strcmp(cmd, "reset")) {
            t.reset();
            withheld.clear();
            have_open = false;
            continue;
        }
        if (!strcmp(cmd, "state")) {
            printf("state %u %u %u %u %u %u\n", t.len_spec, t.len_plain, t.n_spec, t.n_plain, t.probe_pending, t.left);
            continue;
        }
        if (strcmp(cmd, "frames") || sscanf(line, "%*s %u %31s", &n, mode) != 2 ||
            (strcmp(mode, "deliver") && strcmp(mode, "withhold") && strcmp(mode, "open"))) {
            fprintf(stderr, "spec_tuner_driver: bad command: %s", line);
            return 2;
        }
        for (unsigned i = 0; i < n; ++i) {
            const bool must_wait = t.must_wait_for_probe();
            if (must_wait) flush();
            const bool spec = t.next_frame();
            const bool bracketed = t.bracketed(), probe = bracketed && t.probing();
            printf("%u %s %d %d %d %d %d\n", t.frame_no, names[t.phase], (int)spec, (int)bracketed, (int)probe, (int)must_wait, (int)t.leaves_windows(lanes));
            if (!bracketed) continue;
            if (probe) t.probe_opened();
            const Timing tm{spec, probe, spec ? ms_spec : ms_plain};
            if (!strcmp(mode, "deliver")) t.timing(tm.spec, tm.probe, tm.ms);
            else if (!strcmp(mode, "withhold")) withheld.push_back(tm);
            else open = tm, have_open = true;
        }
    }
    return 0;
}
