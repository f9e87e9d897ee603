// spec_tuner.h — the rules of the speculation tuner, free of HIP: arithmetic state and decisions only, so that they run (and are
// tested, tests/test_spec_tuner_cpu.py) on a CPU.  The events that feed it their timings belong to SpecTuner (gsx_state.h) and
// gsx_frame.cpp; a line that decides something belongs here.
//
// ---- does speculating pay on THIS scene, along THIS camera path?  Measured, not guessed. ----
// Temporal occlusion speculation wins when frames are coherent and the scene occludes (cfg4: 2x), and loses when most frames
// need the repair round anyway (cfg2: 1 M sparse Gaussians, 90 % of the frames repair; random camera poses).  Either path
// gives the same pixels, so the viewer simply times them: some frames are bracketed by a pair of HIP events (recorded on the
// stream, read back when they have completed; the host waits for none of them except a probe's, eight frames after it —
// kSettleWait), one running mean per mode, and a four-phase cycle per model:
//   SPEC (len_spec frames) -> PROBE_PLAIN (5 frames, unspeculated; the windows keep being updated) -> SETTLE (speculated
//   frames until the probe's timings have arrived) -> decide;   PLAIN -> PROBE_SPEC -> SETTLE -> decide likewise.
// A decision that confirms the current mode doubles its phase — quadruples it when the verdict is clear — (64 ... 2048
// frames: the probes then cost < 1 %), one that flips it starts over at 64.  By construction the result stays within a few per cent of the better of the two paths.
#pragma once
#include <algorithm>
#include <cstdint>

namespace gsx {

constexpr uint32_t kProbeFrames = 5;   // the first is not timed (the switch itself is atypical), the other four are
constexpr uint32_t kSettleWait = 8;    // frames enqueued behind a probe before the host waits for its timings
constexpr uint32_t kSettleFrames = 64; // at most this many frames between a probe and the decision it feeds (normally: until its timings are in)

struct SpecTunerRules {
    enum Phase { SPEC, PROBE_PLAIN, SETTLE_SPEC, PLAIN, PROBE_SPEC, SETTLE_PLAIN } phase = SPEC;
    uint32_t left = 32;                 // frames left in the phase (the first SPEC phase is short: decide early)
    uint32_t len_spec = 64, len_plain = 64, frame_no = 0;
    double mean_spec = 0.0, mean_plain = 0.0;  // running means of the bracketed frames, milliseconds
    uint32_t n_spec = 0, n_plain = 0;
    uint32_t probe_pending = 0;         // probe frames whose timings have not arrived yet

    // the scene changed under the model (another mask, new Gaussians): what was measured belongs to the old scene
    void reset() {
        phase = SPEC; left = 32; len_spec = len_plain = 64;
        n_spec = n_plain = 0; mean_spec = mean_plain = 0.0; probe_pending = 0;
    }

    bool settling() const { return phase == SETTLE_SPEC || phase == SETTLE_PLAIN; }
    bool probing() const { return phase == PROBE_PLAIN || phase == PROBE_SPEC; }

    // a bracketed frame's events have completed: ms between them (<= 0: the pair could not be read; a probe still counts as arrived)
    void timing(bool speculated, bool probe, float ms) {
        if (ms > 0.0f) {
            double& mean = speculated ? mean_spec : mean_plain;
            uint32_t& n = speculated ? n_spec : n_plain;
            mean = n == 0 ? ms : mean + 0.25 * (ms - mean);
            n += 1;
        }
        if (probe) probe_dropped();
    }
    // a probe frame's bracket was opened ... and went away without a timing (never closed, or its stop was not recorded)
    void probe_opened() { probe_pending += 1; }
    void probe_dropped() {
        if (probe_pending) probe_pending -= 1;
    }

    // a settle phase ends as soon as the probe's timings are in.  Eight frames after the probe the host stops running ahead
    // until they are: it waits for the probe's last event — with eight frames queued behind it the device never idles, and a
    // host that is dozens of short frames ahead (a 1 M-Gaussian scene on two lanes) would otherwise spend that long in the
    // mode it is about to leave
    bool must_wait_for_probe() const { return settling() && probe_pending && kSettleFrames - left >= kSettleWait; }

    // once per frame of a model that could speculate: on to the next frame; returns whether it speculates.  *decided (nullable): this
    // frame took a decision (the means it was taken on are unchanged; the new phase, SPEC or PLAIN, is its outcome)
    bool next_frame(bool* decided = nullptr) {
        if (decided) *decided = false;
        if (settling() && probe_pending == 0) left = 0;
        if (left == 0) {
            switch (phase) {
                case SPEC:
                    phase = PROBE_PLAIN; left = kProbeFrames;
                    break;
                case PLAIN:
                    phase = PROBE_SPEC; left = kProbeFrames;
                    break;
                // a host that does not wait for the device is several frames ahead of it: the probe's timings arrive while the
                // frames after it are being enqueued, so the decision is taken a dozen frames later, in the old mode meanwhile
                case PROBE_PLAIN:
                    phase = SETTLE_SPEC; left = kSettleFrames;
                    break;
                case PROBE_SPEC:
                    phase = SETTLE_PLAIN; left = kSettleFrames;
                    break;
                case SETTLE_SPEC:
                case SETTLE_PLAIN: {
                    const bool was_spec = phase == SETTLE_SPEC;
                    const bool have = n_spec >= 2 && n_plain >= 2;  // (running means over every bracketed frame so far, newest weighted most)
                    const bool spec_better = have ? (was_spec ? mean_spec <= 1.03 * mean_plain : mean_spec < 0.97 * mean_plain) : was_spec;
                    // a clear verdict (the other path costs half as much again, or more) is asked for again four times later, a close
                    // one twice later: on cfg4 a probe is five frames at twice the cost, on cfg2 the two paths are within 5 %
                    const double ratio = !have ? 1.0 : (spec_better ? mean_plain / std::max(mean_spec, 1e-6) : mean_spec / std::max(mean_plain, 1e-6));
                    const uint32_t grow = ratio >= 1.5 ? 4u : 2u;
                    if (spec_better) {
                        len_spec = was_spec ? std::min<uint32_t>(grow * len_spec, 2048u) : 64u;
                        len_plain = 64;
                        phase = SPEC; left = len_spec;
                    } else {
                        len_plain = was_spec ? 64u : std::min<uint32_t>(grow * len_plain, 2048u);
                        len_spec = 64;
                        phase = PLAIN; left = len_plain;
                    }
                    if (decided) *decided = true;
                    break;
                }
            }
        }
        left -= 1;
        frame_no += 1;
        return phase == SPEC || phase == PROBE_SPEC || phase == SETTLE_SPEC;
    }

    // bracket this frame with events?  every frame of a probe but its first (the switch itself is atypical), every
    // fourth frame otherwise (an event pair costs a few microseconds of stream gap)
    bool bracketed() const { return probing() ? left != kProbeFrames - 1 : (frame_no & 3u) == 0; }

    // deep inside a plain phase nobody reads the windows this frame would leave behind (its last frame does: a probe follows)
    // (with frames in flight every lane needs ITS windows for the probe: the last L frames of the phase keep them)
    bool leaves_windows(uint32_t lanes) const { return !(phase == PLAIN && left >= lanes); }
};

}  // namespace gsx
