// sim.cpp — the Monte-Carlo loop of the reference (src/sim/ldpcsim.cpp:97-263) on top of the batched
// GPU step.  The reference decodes one frame per loop trip and re-evaluates its stop rule after each;
// here a batch of frames of the same noise stream is decoded per launch and the per-frame results are
// then folded in stream order with the reference's rule (sim_fold.hpp), so the counters (frames, fec,
// bec, iters) and every line written are those of a single-threaded reference run with the same seed.
// Frames decoded past the stopping frame are discarded.
#include "sim.hpp"

#include <chrono>
#include <fstream>
#include <iostream>
#include <stdexcept>

#include "sim_fold.hpp"

namespace ldpc_amd
{

namespace
{
// One channel point on one rank: batches of the stream, folded frame by frame; publish(counters) at every frame error.
template <class Publish>
PointCounters run_point(Engine &eng, const SimRequest &rq, const bool *stop_flag, Publish &&publish)
{
    PointCounters pc;
    const uint64_t max_batch = std::min<uint64_t>(rq.max_batch, eng.max_sub_batch());
    const uint64_t min_batch = std::min(rq.first_batch, max_batch);
    std::vector<uint32_t> it_buf, be_buf;
    for (uint64_t batch = min_batch;; batch = next_step(pc, rq.min_fec, rq.max_frames, min_batch, max_batch, /*ladder=*/false))
    {
        it_buf.resize(batch), be_buf.resize(batch);
        BatchOut out;
        out.iters = it_buf.data(), out.bit_errors = be_buf.data();
        eng.stream_decode(rq.dec, batch, out, nullptr);
        // a raised flag ends the reference's do-while after the frame in flight (ldpcsim.cpp:255)
        const bool flagged = *stop_flag;
        const Fold f = fold_range(it_buf.data(), be_buf.data(), flagged ? std::min<uint64_t>(batch, 1) : batch, pc.frames, pc.fec,
                                  rq.min_fec, rq.max_frames, [&](const Fold &g) { publish(pc.plus(g, rq.min_fec)); });
        pc = pc.plus(f, rq.min_fec);
        if (f.stop || flagged)
        {
            // frames decoded past the stopping frame never happened as far as the encoder is concerned
            eng.stream_rewind_encoder(batch - f.n, nullptr);
            return pc;
        }
    }
}

// One channel point over the ranks of comm: every rank folds its share of a step, the folds are reduced in rank order;
// publish(counters) after every step with a frame error.  Every rank returns the same counters.
template <class Publish>
PointCounters run_point_sharded(Engine &eng, const SimRequest &rq, const bool *stop_flag, Comm &comm, Publish &&publish)
{
    PointCounters pc;
    const int R = comm.world(), me = comm.rank();
    const uint64_t msb = eng.max_sub_batch() * 3 / 4; // (a piece may hold a few per cent more frames than its share)
    uint64_t max_step = std::max<uint64_t>(1, std::min<uint64_t>(rq.max_batch, msb)) * R;
    // a piece is at least one whole generator chunk: for very short codes that is more frames than one launch takes, however
    // small the step — such a code is turned away here, with a reason, on every rank alike; otherwise the largest step is
    // brought down to what the output buffers of one launch per rank hold
    while (max_step > static_cast<uint64_t>(R) && eng.shard_capacity(max_step, R) > eng.max_sub_batch())
        max_step = std::max<uint64_t>(R, max_step * 3 / 4);
    if (eng.shard_capacity(max_step, R) > eng.max_sub_batch())
        throw std::runtime_error("sharded simulation: one generator chunk of the noise stream holds more frames of this code than one "
                                 "launch takes (very short code): run it on one rank, or with a smaller LDPC_AMD_CHUNK_BLOCKS");
    const uint64_t min_step = std::min<uint64_t>(rq.first_batch, max_step);
    std::vector<uint32_t> it_buf, be_buf;
    std::vector<Fold> all(static_cast<size_t>(R));
    for (uint64_t step = min_step;; step = next_step(pc, rq.min_fec, rq.max_frames, min_step, max_step, /*ladder=*/true))
    {
        const uint64_t cap = eng.shard_capacity(step, R);
        it_buf.resize(cap), be_buf.resize(cap);
        BatchOut out;
        out.iters = it_buf.data(), out.bit_errors = be_buf.data();
        // A rank whose step fails (a HIP error, a device that went away) still takes part in the exchange below and says
        // so in the last word: every rank then leaves the loop with an error instead of waiting for the one that is gone.
        Engine::ShardStep st;
        std::string step_error;
        Fold mine;
        // (the encoder snapshot comes before the step's own exchange: if it fails here, the step is entered with the failure
        // in hand so that this rank still takes part in that exchange instead of going straight to the one below while the
        // other ranks sit in the step's)
        std::string snap_error;
        try
        {
            eng.encoder_snapshot(nullptr);
        }
        catch (const std::exception &e)
        {
            snap_error = e.what();
        }
        try
        {
            st = eng.stream_decode_sharded(comm, rq.dec, step, out, nullptr, snap_error.empty() ? nullptr : &snap_error);
            // every rank's range as if all of it counted; the ranks before the one holding the stopping frame do
            mine = fold_range(it_buf.data(), be_buf.data(), st.n, 0, 0, kNoLimit, kNoLimit);
        }
        catch (const std::exception &e)
        {
            step_error = e.what();
        }
        mine.stop = *stop_flag ? 1 : 0, mine.failed = step_error.empty() ? 0 : 1;
        comm.all_gather(&mine, all.data(), sizeof mine);
        bool flagged = false;
        for (int q = 0; q < R; ++q)
        {
            if (all[q].failed)
                throw std::runtime_error(q == me ? "sharded simulation: " + step_error
                                                 : "sharded simulation: the step failed on rank " + std::to_string(q));
            flagged = flagged || all[q].stop;
        }
        const uint64_t rep_before = pc.rep_frames;
        uint64_t used = 0;
        const int q_stop = reduce_ranks(all.data(), R, pc, rq.min_fec, rq.max_frames, &used);
        if (q_stop >= 0)
        {
            // the owner of the stopping frame walks its range again from the state the ranks before it leave
            Fold cut;
            if (q_stop == me)
                cut = fold_range(it_buf.data(), be_buf.data(), st.n, pc.frames, pc.fec, rq.min_fec, rq.max_frames);
            comm.all_gather(&cut, all.data(), sizeof cut);
            apply_cut(all[q_stop], pc, rq.min_fec, &used);
        }
        const bool done = q_stop >= 0 || flagged;
        if (done)
            eng.encoder_restore_and_skip(used, nullptr); // the encoder stands after the stopping frame, on every rank
        if (pc.rep_frames != rep_before)
            publish(pc);
        if (done)
            return pc;
    }
}
} // namespace

int run_simulation(Engine &eng, const SimRequest &rq, sim_results_t *results, uint64_t *totals, bool *stop_flag, Comm *comm)
{
    using clock = std::chrono::high_resolution_clock;
    static bool never_stop = false;
    if (!stop_flag)
        stop_flag = &never_stop;
    const bool sharded = comm && comm->world() > 1;
    const bool root = !sharded || comm->rank() == 0; // rank 0 prints and writes
    const std::vector<double> xs = channel_points(rq.x_range, rq.channel);
    std::vector<std::string> lines(xs.size() + 1);
    if (rq.cli_output)
        lines[0] = "snr fer ber frames avg_iter frame_time";
    if (root)
    {
        std::cout << "=============================" << "===========================================================" << std::endl;
        std::cout << "  FEC   |      FRAME     |   " << (eps_axis(rq.channel) ? "EPS" : "SNR")
                  << "   |    BER     |    FER     | AVGITERS  |  TIME/FRAME   \n";
        std::cout << "========+================+===" << "======+============+============+===========+==============" << std::endl;
    }
    const uint64_t nc = static_cast<uint64_t>(eng.code().nc());
    for (size_t i = 0; i < xs.size(); ++i)
    {
        auto t_start = clock::now();
        // the reference's report at a frame error (ldpcsim.cpp:192-251)
        const auto publish = [&](const PointCounters &pc) {
            const auto t_now = clock::now();
            const uint64_t us = static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::microseconds>(t_now - t_start).count());
            const Report r = make_report(xs[i], pc, rq.min_fec, nc, us / pc.rep_frames);
            if (rq.cli_output && root)
            {
                std::fputs(r.console.c_str(), stdout);
                std::fflush(stdout);
                lines[i + 1] = r.file_line;
                std::ofstream fp(rq.result_file);
                if (fp.good())
                    for (const auto &l : lines)
                        fp << l << "\n";
                else
                    std::printf("Warning: can not open logfile for writing\n");
            }
            if (results)
            {
                results->fer[i] = r.fer, results->ber[i] = r.ber, results->avg_iter[i] = r.avg_iter;
                results->time[i] = r.time, results->fec[i] = r.fec, results->frames[i] = r.frames;
            }
            t_start += clock::now() - t_now; // printing is not charged to the frame time
        };
        // the reference builds its channel objects once per run (ldpcsim.cpp:29-75): the info-word stream
        // and the accumulated codeword carry over from one channel point to the next
        eng.stream_begin(rq.channel, rq.seed, xs[i], /*fresh=*/i == 0);
        const PointCounters pc = sharded ? run_point_sharded(eng, rq, stop_flag, *comm, publish) : run_point(eng, rq, stop_flag, publish);
        if (rq.cli_output && root)
            std::printf("\n");
        if (totals)
        {
            totals[4 * i + 0] = pc.frames, totals[4 * i + 1] = pc.fec;
            totals[4 * i + 2] = pc.bec, totals[4 * i + 3] = pc.iters;
        }
    }
    return static_cast<int>(xs.size());
}

} // namespace ldpc_amd
