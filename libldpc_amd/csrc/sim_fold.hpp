// sim_fold.hpp — the counters, the stop rule and the report of the reference's Monte-Carlo loop (src/sim/ldpcsim.cpp:97-263)
// as host arithmetic over per-frame results: no GPU, no communicator, no clock.  sim.cpp drives the engine with it, and
// ldpc_hip_selftest_sim_fold (api.cpp) runs the same functions over given arrays for the CPU tests.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace ldpc_amd
{

// What folding a range of consecutive frames adds to a channel point's counters.  It is also a rank's row of a sharded
// step's exchange, eight words: `stop` then carries the rank's stop flag (first exchange) or "the rule fired" (second),
// `failed` that the rank's step threw.
struct Fold
{
    uint64_t n = 0; // frames walked (the whole range unless the stop rule fired)
    uint64_t fec = 0, bec = 0, iters = 0;
    uint64_t n_at_err = 0;     // frames walked up to and including the last frame error (0: none)
    uint64_t iters_at_err = 0; // iterations summed up to and including that frame
    uint64_t stop = 0;         // the stop rule fired at frame n
    uint64_t failed = 0;
};
static_assert(sizeof(Fold) == 8 * sizeof(uint64_t), "a Fold is a row of the exchange");

constexpr uint64_t kNoLimit = ~0ull;

// One channel point.  A report is made at a frame error and only there, and fec and bec change only there: the last
// report's fec and bec are the running ones, its frames and iterations are kept (rep_frames == 0: no report yet).
struct PointCounters
{
    uint64_t frames = 0, fec = 0, bec = 0, iters = 0;
    uint64_t rep_frames = 0, rep_iters = 0;

    // these counters after a fold that started from their (frames, fec).  Frames are counted only while fec < min_fec
    // (ldpcsim.cpp:178), which within a fold can only fail at its first frame: the rule stops a fold at the frame that
    // brings fec up to min_fec.
    PointCounters plus(const Fold &f, uint64_t min_fec) const
    {
        PointCounters p = *this;
        if (f.fec > 0)
            p.rep_frames = frames + f.n_at_err, p.rep_iters = iters + f.iters_at_err;
        if (fec < min_fec)
            p.frames += f.n;
        p.fec += f.fec, p.bec += f.bec, p.iters += f.iters;
        return p;
    }
};

// ldpcsim.cpp:175-255 over `count` consecutive frames, starting from `frames0` counted frames and `fec0` frame errors: the
// iterations of every frame are added (:176), a frame and its errors are counted only while fec < min_fec (:178), the rule
// of :255 is evaluated after every frame.  on_error(fold so far) is called at every frame error (the reference's report).
struct NoReport { void operator()(const Fold &) const {} };

template <class OnError = NoReport>
Fold fold_range(const uint32_t *it, const uint32_t *be, uint64_t count, uint64_t frames0, uint64_t fec0, uint64_t min_fec,
                uint64_t max_frames, OnError &&on_error = {})
{
    Fold f;
    uint64_t counted = 0;
    for (uint64_t i = 0; i < count && !f.stop; ++i)
    {
        f.n = i + 1;
        f.iters += it[i];
        if (fec0 + f.fec < min_fec)
        {
            ++counted;
            if (be[i] > 0)
            {
                f.bec += be[i];
                ++f.fec;
                f.n_at_err = f.n, f.iters_at_err = f.iters;
                on_error(f);
            }
        }
        f.stop = !(fec0 + f.fec < min_fec && frames0 + counted < max_frames);
    }
    return f;
}

// A sharded step, first half: rows[q] is rank q's fold of its whole range with no limits (fold_range(.., 0, 0, kNoLimit,
// kNoLimit)), in stream order.  Returns the rank inside whose range (or at whose end) the rule fires, -1 if it does not
// fire in this step, and advances pc over the ranks before that one (all of them for -1); *used grows by their frames.
// A rank without frames cannot hold the stopping frame: at a step's start (min_fec == 0, max_frames == 0) the reference
// still decodes one frame, which is the first frame of the first rank that has one.
inline int reduce_ranks(const Fold *rows, int world, PointCounters &pc, uint64_t min_fec, uint64_t max_frames, uint64_t *used)
{
    for (int q = 0; q < world; ++q)
    {
        const Fold &L = rows[q];
        if (L.n > 0 && (pc.fec + L.fec >= min_fec || pc.frames + L.n >= max_frames))
            return q;
        pc = pc.plus(L, min_fec);
        *used += L.n;
    }
    return -1;
}

// second half: `cut` is the stopping rank's fold of its range from the state reduce_ranks left, with the limits
// (fold_range(.., pc.frames, pc.fec, min_fec, max_frames))
inline void apply_cut(const Fold &cut, PointCounters &pc, uint64_t min_fec, uint64_t *used)
{
    pc = pc.plus(cut, min_fec);
    *used += cut.n;
}

// ldpcsim.cpp:202-217 and :243-248 at the last frame error of pc; t_frame_us as the reference's tFrame
struct Report
{
    std::string console, file_line;
    double fer, ber, avg_iter, time;
    uint64_t fec, frames;
};

inline Report make_report(double x, const PointCounters &pc, uint64_t min_fec, uint64_t nc, uint64_t t_frame_us)
{
    Report r;
    r.fec = pc.fec, r.frames = pc.rep_frames;
    r.fer = static_cast<double>(pc.fec) / pc.rep_frames;
    r.ber = static_cast<double>(pc.bec) / (pc.rep_frames * nc); // nc, not nct (ldpcsim.cpp:205)
    r.avg_iter = static_cast<double>(pc.rep_iters) / pc.rep_frames;
    r.time = static_cast<double>(t_frame_us) * 1e-6;
    char buf[200];
    std::snprintf(buf, sizeof buf, "\r %2lu/%2lu  |  %12lu  |  %.3f  |  %.2e  |  %.2e  |  %.1e  |  %.3fms", pc.fec, min_fec,
                  pc.rep_frames, x, r.ber, r.fer, r.avg_iter, static_cast<double>(t_frame_us) * 1e-3);
    r.console = buf;
    std::snprintf(buf, sizeof buf, "%lf %.3e %.3e %lu %.3e %.6f", x, r.fer, r.ber, pc.rep_frames, r.avg_iter, r.time);
    r.file_line = buf;
    return r;
}

// BSC (2) and BEC (3), in the reference's channel_type numbering (ldpcsim.h:15-20), have an epsilon axis, AWGN (1) an SNR axis
inline bool eps_axis(int channel) { return channel == 2 || channel == 3; }

// channel points MIN, MIN+STEP, ... < MAX (ldpcsim.cpp:104-110); worst point first on an epsilon axis (:116-122)
inline std::vector<double> channel_points(const double x_range[3], int channel)
{
    std::vector<double> xs;
    for (double v = x_range[0]; v < x_range[1]; v += x_range[2])
        xs.push_back(v);
    if (eps_axis(channel))
        std::reverse(xs.begin(), xs.end());
    return xs;
}

// Frames of the next step while the rule has not fired: enough for the errors still missing at the observed rate, within
// [min_step, max_step].  ladder: one of a few sizes only (powers of two times min_step, and max_step) — in a sharded step
// every new size is a new piece geometry: jump polynomials multiplied on the host, a table re-seek.
inline uint64_t next_step(const PointCounters &pc, uint64_t min_fec, uint64_t max_frames, uint64_t min_step, uint64_t max_step,
                          bool ladder)
{
    uint64_t want = max_step;
    if (pc.fec > 0)
    {
        const double per_err = static_cast<double>(pc.frames) / static_cast<double>(pc.fec);
        want = static_cast<uint64_t>(per_err * static_cast<double>(min_fec - pc.fec) * 1.25) + 1;
    }
    want = std::min<uint64_t>(want, max_frames - pc.frames);
    if (!ladder)
        return std::clamp<uint64_t>(want, min_step, max_step);
    uint64_t q = min_step;
    while (q < want && q < max_step)
        q = std::min<uint64_t>(q * 2, max_step);
    return q;
}

} // namespace ldpc_amd
