// engine.cpp — see engine.hpp.  Compiled by hipcc (host code using the HIP runtime API).
#include "engine.hpp"
#include "shard_place.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>

namespace ldpc_amd
{

std::string hip_error_string(int err) { return hipGetErrorString(static_cast<hipError_t>(err)); }

namespace
{
void check(hipError_t e, const char *what)
{
    if (e != hipSuccess)
        throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}
void check(int e, const char *what) { check(static_cast<hipError_t>(e), what); }

bool is_device_ptr(const void *p)
{
    if (!p)
        return false;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess)
    {
        (void)hipGetLastError(); // plain host memory: clear the sticky error
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

} // namespace

// routes an output either straight to the caller's device pointer or through a staging buffer
struct OutStage
{
    struct Item
    {
        void *host, *dev;
        size_t bytes;
    };
    std::vector<Item> items;
    template <typename T>
    T *route(T *user, DeviceBuffer &stage, size_t bytes)
    {
        if (!user)
            return nullptr;
        if (is_device_ptr(user))
            return user;
        void *d = stage.reserve(bytes);
        items.push_back({user, d, bytes});
        return static_cast<T *>(d);
    }
    size_t pinned_bytes() const
    {
        size_t total = 0;
        for (auto &i : items)
            total += (i.bytes + 63) & ~size_t(63);
        return total;
    }
    // small results go through page-locked memory: a device-to-pageable copy is a blocking staged copy per call,
    // which is most of a single-frame decode()'s latency.  `word` (optional): a device word that rides along and is
    // returned — the results are delivered, the items kept, so that the caller can deliver them again after more launches.
    uint32_t flush(hipStream_t s, PinnedBuffer *pin = nullptr, const uint32_t *word = nullptr)
    {
        const size_t total = pinned_bytes();
        if (pin && total && total <= kPinnedLimit)
        {
            char *h = static_cast<char *>(pin->reserve(total + 64));
            size_t off = 0;
            for (auto &i : items)
            {
                check(hipMemcpyAsync(h + off, i.dev, i.bytes, hipMemcpyDeviceToHost, s), "copy out");
                off += (i.bytes + 63) & ~size_t(63);
            }
            if (word)
                check(hipMemcpyAsync(h + total, word, 4, hipMemcpyDeviceToHost, s), "copy out");
            check(hipStreamSynchronize(s), "sync");
            off = 0;
            for (auto &i : items)
            {
                std::memcpy(i.host, h + off, i.bytes);
                off += (i.bytes + 63) & ~size_t(63);
            }
            if (word)
            {
                uint32_t w;
                std::memcpy(&w, h + total, 4);
                return w;
            }
            items.clear();
            return 0;
        }
        if (word)
            throw std::runtime_error("OutStage: a ride-along word needs the page-locked path");
        for (auto &i : items)
            check(hipMemcpyAsync(i.host, i.dev, i.bytes, hipMemcpyDeviceToHost, s), "copy out");
        if (!items.empty())
            check(hipStreamSynchronize(s), "sync");
        items.clear();
        return 0;
    }
    static constexpr size_t kPinnedLimit = 1 << 20;
};

// ---------------------------------------------------------------------------------------------
PinnedBuffer::~PinnedBuffer()
{
    if (ptr_)
        (void)hipHostFree(ptr_);
}

void *PinnedBuffer::reserve(size_t bytes)
{
    if (bytes > size_)
    {
        if (ptr_)
            check(hipHostFree(ptr_), "hipHostFree");
        ptr_ = nullptr;
        const size_t want = std::max<size_t>(bytes, 64 * 1024);
        check(hipHostMalloc(&ptr_, want, hipHostMallocDefault), "hipHostMalloc");
        size_ = want;
    }
    return ptr_;
}

DeviceBuffer::~DeviceBuffer()
{
    if (ptr_)
        (void)hipFree(ptr_);
}

void *DeviceBuffer::reserve(size_t bytes)
{
    if (bytes > size_)
    {
        if (ptr_)
            check(hipFree(ptr_), "hipFree");
        ptr_ = nullptr;
        // an eighth of slack from the first allocation on: the per-batch buffers of the noise stream follow the number of
        // chunks a batch spans, which varies by one or two in eighty, and growing means hipFree — a wait for everything
        // the device has in flight, the decode kernel of the batch before included (it cost a 4 ms step 2 ms whenever a
        // batch set a new maximum: steps 1, 3, 52 and 64 of the headline run)
        size_t want = std::max(bytes + bytes / 8, size_ + size_ / 2);
        check(hipMalloc(&ptr_, want), "hipMalloc");
        size_ = want;
    }
    return ptr_;
}

// ---------------------------------------------------------------------------------------------
MtDevice::MtDevice()
{
    // 1120 blocks = 349 440 words = 2.8 MB of raw stream per chunk: the serial twist chain of a chunk has to hide under the
    // decode kernel, whose waves outrank it.  Round 3's headline kernel (3.6 ms) hid chunks of 2240 blocks; under round 4's
    // (2.6 ms) their chain outlasts it (step 2.95 ms), chunks of 840..1400 blocks all give 2.76..2.79 ms, and at 560 the
    // jump-ahead tasks (one per chunk, two steps ahead) take over.  A 65 536-frame batch spans 165 chunks.
    // LDPC_AMD_CHUNK_BLOCKS: experiments / tests of the chunk edges.
    chunk_blocks_ = 1120;
    if (const char *e = std::getenv("LDPC_AMD_CHUNK_BLOCKS"))
    {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= (1 << 20))
            chunk_blocks_ = static_cast<uint32_t>(v), chunk_blocks_from_env_ = true;
    }
}

MtDevice::~MtDevice()
{
    if (jump_stream_)
    {
        (void)hipStreamSynchronize(static_cast<hipStream_t>(jump_stream_));
        (void)hipStreamDestroy(static_cast<hipStream_t>(jump_stream_));
    }
    for (Ahead &a : ahead_)
        (void)hipEventDestroy(static_cast<hipEvent_t>(a.event));
    for (void *e : ev_free_)
        (void)hipEventDestroy(static_cast<hipEvent_t>(e));
    if (ev_main_)
        (void)hipEventDestroy(static_cast<hipEvent_t>(ev_main_));
    for (void *e : ev_strided_)
        if (e)
            (void)hipEventDestroy(static_cast<hipEvent_t>(e));
    for (auto &p : polys_)
        if (p.second)
            (void)hipFree(p.second);
}

void MtDevice::reset(uint64_t seed)
{
    if (seeded_ && seed == seed_)
        return; // chunk states depend on the seed only; keep them
    seed_ = seed;
    seeded_ = true;
    if (jump_stream_) // look-ahead launches of the old seed: done before the ring is written again
        check(hipStreamSynchronize(static_cast<hipStream_t>(jump_stream_)), "sync");
    for (Ahead &a : ahead_)
        ev_free_.push_back(a.event);
    ahead_.clear();
    for (bool &b : strided_pending_)
        b = false;
    ring_.invalidate();
    strided_.invalidate();
}

// device copy of t^(312 * chunk_blocks * stride) mod phi, uploaded once per stream object and stride
const uint64_t *MtDevice::device_poly(uint64_t stride, void *stream)
{
    for (auto &p : polys_)
        if (p.first == stride)
            return static_cast<const uint64_t *>(p.second);
    // bounded: beyond 64 device copies the older half goes, except the ring's powers of two (launches that read them may be
    // in flight: the device is drained first — once per 32 new step geometries of a simulation, if ever)
    if (polys_.size() >= 64)
    {
        check(hipDeviceSynchronize(), "sync before trimming the polynomial cache");
        std::vector<std::pair<uint64_t, void *>> keep;
        for (size_t i = 0; i < polys_.size(); ++i)
            if (i >= polys_.size() / 2 || (polys_[i].first & (polys_[i].first - 1)) == 0)
                keep.push_back(polys_[i]);
            else
                (void)hipFree(polys_[i].second);
        polys_.swap(keep);
    }
    const Gf2Poly &g = chunk_jump_poly(chunk_blocks_, stride);
    std::vector<uint64_t> padded(kJumpPolyWords, 0);
    std::copy(g.begin(), g.begin() + kMtWords, padded.begin());
    void *d = nullptr;
    check(hipMalloc(&d, sizeof(uint64_t) * kJumpPolyWords), "hipMalloc poly");
    polys_.emplace_back(stride, d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    check(hipMemcpyAsync(d, padded.data(), sizeof(uint64_t) * kJumpPolyWords, hipMemcpyHostToDevice, s), "upload poly");
    check(hipStreamSynchronize(s), "sync"); // `padded` is a local buffer
    return static_cast<const uint64_t *>(d);
}

void MtDevice::apply(const std::vector<StateOp> &ops, uint64_t *table, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t row = sizeof(uint64_t) * kMtWords;
    for (const StateOp &op : ops)
        switch (op.kind)
        {
        case StateOp::kUpload0:
        {
            uint64_t w0[kMtWords];
            mt64_window0(seed_, w0);
            check(hipMemcpyAsync(table + static_cast<size_t>(op.dst) * kMtWords, w0, row, hipMemcpyHostToDevice, s), "upload window0");
            check(hipStreamSynchronize(s), "sync"); // w0 is a stack buffer
            break;
        }
        case StateOp::kCopy:
            check(hipMemcpyAsync(table + static_cast<size_t>(op.dst) * kMtWords, table + static_cast<size_t>(op.src) * kMtWords, row,
                                 hipMemcpyDeviceToDevice, s),
                  "state copy");
            break;
        case StateOp::kJump:
            check(launch_mt_jump(table, op.mod, op.src, op.dst, device_poly(op.stride, stream), op.n, jump_groups_, s), "mt_jump");
            jump_tasks_ += op.n;
            break;
        }
}

uint32_t MtDevice::ensure_ring(uint64_t c_lo, uint64_t c_hi, void *stream)
{
    uint64_t *table = static_cast<uint64_t *>(ring_buf_.reserve(sizeof(uint64_t) * kMtWords * StateRing::kTotalRows));
    if (!ring_polys_ready_)
    {
        // every stride the ring will ever use (the powers of two up to its window), computed and uploaded NOW: a
        // polynomial squaring takes the host 10 ms, and the ring's window reaches its full width only after two dozen
        // batches — inside somebody's timed region
        for (uint32_t w = 1; w <= StateRing::kWindow; w *= 2)
            (void)device_poly(w, stream);
        ring_polys_ready_ = true;
    }
    std::vector<StateOp> ops;
    ring_.ensure(c_lo, c_hi, ops);
    // Look-ahead launches (prefetch_ring) in flight: the request waits for those that wrote a row it reads; operations
    // planned here (a seek, an extension the look-ahead did not cover) read and write rows anywhere: they wait for all.
    drain_ahead(stream, ops.empty() ? c_hi : ~0ull);
    apply(ops, table, stream);
    if (!ops.empty())
    {
        if (!ev_main_)
        {
            hipEvent_t e;
            check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
            ev_main_ = e;
        }
        check(hipEventRecord(static_cast<hipEvent_t>(ev_main_), static_cast<hipStream_t>(stream)), "event");
        main_dirty_ = true;
    }
    return static_cast<uint32_t>(c_lo % StateRing::kRows);
}

void MtDevice::drain_ahead(void *stream, uint64_t below)
{
    size_t n = 0;
    while (n < ahead_.size() && ahead_[n].hi_before < below)
        ++n;
    if (n == 0)
        return;
    // (one stream, in order: the newest of them implies the others)
    check(hipStreamWaitEvent(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(ahead_[n - 1].event), 0), "wait look-ahead");
    for (size_t i = 0; i < n; ++i)
        ev_free_.push_back(ahead_[i].event); // (re-recorded only after this wait has been enqueued: safe to reuse)
    ahead_.erase(ahead_.begin(), ahead_.begin() + static_cast<std::ptrdiff_t>(n));
}

void MtDevice::prefetch_ring(uint64_t c_hi)
{
    if (!ring_.valid() || !ring_polys_ready_)
        return;
    const uint64_t hi_before = ring_.hi();
    std::vector<StateOp> ops;
    ring_.extend_to(c_hi, ops);
    if (ops.empty())
        return;
    if (!jump_stream_)
    {
        hipStream_t js;
        check(hipStreamCreateWithFlags(&js, hipStreamNonBlocking), "hipStreamCreate");
        jump_stream_ = js;
    }
    hipStream_t js = static_cast<hipStream_t>(jump_stream_);
    if (main_dirty_) // rows written on the caller's stream (the seek, the first extensions) are sources here
    {
        check(hipStreamWaitEvent(js, static_cast<hipEvent_t>(ev_main_), 0), "wait ring");
        main_dirty_ = false;
    }
    apply(ops, ring(), js);
    void *ev;
    if (!ev_free_.empty())
        ev = ev_free_.back(), ev_free_.pop_back();
    else
    {
        hipEvent_t e;
        check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
        ev = e;
    }
    check(hipEventRecord(static_cast<hipEvent_t>(ev), js), "event");
    ahead_.push_back({hi_before, ring_.hi(), ev});
}

uint64_t *MtDevice::ensure_strided(uint64_t first, uint32_t n, uint64_t stride, void *stream)
{
    uint64_t *table = static_cast<uint64_t *>(strided_buf_.reserve(sizeof(uint64_t) * kMtWords * StridedTable::kTotalRows));
    std::vector<StateOp> ops;
    const uint32_t base = strided_.position(first, n, stride, ops);
    // a look-ahead launch wrote the table that is read now; operations planned here may touch any table: they wait for all
    for (uint32_t k = 0; k < StridedTable::kSlots; ++k)
        if (strided_pending_[k] && (k == base / StridedTable::kMaxRows || !ops.empty()))
        {
            check(hipStreamWaitEvent(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(ev_strided_[k]), 0), "wait look-ahead");
            strided_pending_[k] = false;
        }
    apply(ops, table, stream);
    if (!ops.empty())
    {
        if (!ev_main_)
        {
            hipEvent_t e;
            check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
            ev_main_ = e;
        }
        check(hipEventRecord(static_cast<hipEvent_t>(ev_main_), static_cast<hipStream_t>(stream)), "event");
        main_dirty_ = true;
    }
    return table + static_cast<size_t>(base) * kMtWords;
}

void MtDevice::prefetch_strided()
{
    if (!strided_buf_.get())
        return;
    std::vector<StateOp> ops;
    strided_.look_ahead(ops);
    if (ops.empty())
        return;
    if (!jump_stream_)
    {
        hipStream_t js;
        check(hipStreamCreateWithFlags(&js, hipStreamNonBlocking), "hipStreamCreate");
        jump_stream_ = js;
    }
    hipStream_t js = static_cast<hipStream_t>(jump_stream_);
    if (main_dirty_)
    {
        check(hipStreamWaitEvent(js, static_cast<hipEvent_t>(ev_main_), 0), "wait table");
        main_dirty_ = false;
    }
    for (const StateOp &op : ops) // one launch per table, its event for the step that reads that table
    {
        apply({op}, static_cast<uint64_t *>(strided_buf_.get()), js);
        const uint32_t k = op.dst / StridedTable::kMaxRows;
        if (!ev_strided_[k])
        {
            hipEvent_t e;
            check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
            ev_strided_[k] = e;
        }
        check(hipEventRecord(static_cast<hipEvent_t>(ev_strided_[k]), js), "event");
        strided_pending_[k] = true;
    }
}

const uint64_t *MtStream::generate(uint64_t first, uint64_t count, void *stream, int buffer)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (count == 0)
        count = 1;
    const uint64_t cw = st.chunk_words();
    const uint64_t c_lo = first / cw;
    const uint64_t c_hi = (first + count + cw - 1) / cw;
    if (c_hi - c_lo > StateRing::kWindow)
        throw std::runtime_error("mt19937_64 stream request exceeds the chunk-state window");
    const uint32_t row = st.ensure_ring(c_lo, c_hi, stream);
    const uint32_t n = static_cast<uint32_t>(c_hi - c_lo);
    uint64_t *raw = static_cast<uint64_t *>(raw_[buffer & 1].reserve(sizeof(uint64_t) * cw * n));
    uint32_t words = static_cast<uint32_t>(cw);
    if (n == 1)
    {
        // a short request inside one chunk (single frames, small batches): only the prefix of the chunk that is asked
        // for is generated (whole twist rounds of 312 words)
        const uint64_t need = (first + count - c_lo * cw + kMtWords - 1) / kMtWords * kMtWords;
        words = static_cast<uint32_t>(std::min<uint64_t>(need, cw));
    }
    check(launch_mt_generate(st.ring(), MtDevice::ring_rows(), row, raw, n, words, words, n == 1 ? 1 : pack_, s), "mt_generate");
    // a reader going through the stream front to back (one rank: every request starts where the one before ended): the
    // chunk start states of the next request but one, now (MtDevice::prefetch_ring).  A rank of a sharded stream reads its
    // share of every step, a fixed distance apart: nothing to look ahead for, the ring moves by that distance in one launch.
    if (first == last_end_ && n > 1)
        st.prefetch_ring(c_hi + 2 * (static_cast<uint64_t>(n) + 1));
    last_end_ = first + count;
    return raw + (first - c_lo * cw);
}

// ---------------------------------------------------------------------------------------------
Engine::Engine(const std::string &pc_file, const std::string &gen_file, int device) : device_(device)
{
    code_ = std::make_unique<LdpcCode>(pc_file, gen_file);
    if (code_->min_cn_degree() < 2)
        throw std::runtime_error("check nodes of degree < 2 are not supported (undefined in the reference decoder)");
    plan_ = build_plan(*code_);
    // the device plan's sizes: known before anything is uploaded (refusal reads them on the host)
    dev_.nc = plan_.nc, dev_.mc = plan_.mc, dev_.nnz = plan_.nnz, dev_.nct = plan_.nct;
    dev_.n_bitpos = plan_.n_bitpos;
    dev_.n_cn_blocks = static_cast<int>(plan_.cn_blocks.size());
    dev_.n_vn_blocks = static_cast<int>(plan_.vn_blocks.size());
    dev_.cn_work_stride = plan_.cn_work_stride, dev_.vn_work_stride = plan_.vn_work_stride;
    const size_t nc = plan_.nc, nnz = plan_.nnz;
    if (plan_.lds_ok)
    {
        residency_ = Residency::kLds;
        fused_plan_ = build_fused_plan(*code_, plan_);
        // Input LLRs: in registers when that frees the LDS for one more resident frame per CU (n=1024 code: 40 KB -> 31 KB,
        // five frames instead of four) and the plan allows it; in LDS otherwise.  (Device memory also reached five frames
        // but paid for it in memory reads: measured, no net gain.)
        const size_t cu_lds = kCuLdsBytes, with_llr = plan_.lds_bytes, without = plan_.lds_bytes - 8 * nc;
        if (cu_lds / without > cu_lds / with_llr && plan_.vn_work_stride <= 8 && !plan_.has_isolated_vn && plan_.nc <= plan_.nnz &&
            !plan_.vn_packed.empty())
            lds_llr_mode_ = 2;
        return;
    }
    for (int r = 0; r < code_->H.rows && !shared6_; ++r)
        shared6_ = code_->H.rptr[r + 1] - code_->H.rptr[r] == 6;
    // register-resident decoder: the smallest register tile the code fits.  One frame per CU (1024 threads, 128 VGPRs,
    // 160 KB mailbox) first: measured 1.37x faster on the n=8192 code than two frames per CU (512 threads, 256 VGPRs, 80 KB
    // mailboxes, one more exchange round), which remains for tiles that do not fit 128 registers.
    struct Tile { int nt, kc, maxd; };
    for (Tile t : {Tile{1024, 4, 6}, Tile{1024, 8, 4}, Tile{1024, 2, 8}, Tile{512, 8, 6}, Tile{512, 16, 4}, Tile{512, 4, 8}})
    {
        reg_plan_ = build_reg_plan(*code_, plan_, t.nt, t.kc, t.maxd, t.nt == 512 ? 80 * 1024 : kCuLdsBytes);
        if (reg_plan_.ok)
            break;
    }
    if (reg_plan_.ok)
    {
        // second form (totals come back instead of messages): preferred when the code fits its one instantiation
        reg2_plan_ = build_reg2_plan(*code_, plan_, 1024, 4, 6, 4, 4);
        residency_ = reg2_plan_.ok ? Residency::kRegTotals : Residency::kRegMessages;
        // a register-resident decode workgroup owns its CU: keep the noise generator of the next batch, which runs
        // beside it, on a quarter of the CUs (config 4: 4.89 -> 4.62 ms per step)
        // ... and in chunks of 2240 blocks: half as many jump-ahead tasks per batch as the LDS-resident decoders' 1120 — here
        // every task holds a CU that a frame could have, and the generator's longer chain still ends before the 4.6 ms launch
        noise_.set_pack(4), noise_.st.set_default_chunk_blocks(2240);
    }
    else if (plan_.hbm_ok)
    {
        residency_ = Residency::kMemory;
        // resident frames per CU are bounded through a dummy LDS request so that the frames in flight
        // (256 CUs x frames/CU x state bytes) stay inside the 256 MiB Infinity Cache
        const uint64_t per_frame = 8ull * nnz + 8ull * nc + nnz;
        const uint64_t frames_per_cu = std::clamp<uint64_t>((224ull << 20) / (256 * per_frame), 1, 8);
        mem_occ_lds_ = frames_per_cu >= 8 ? 0 : static_cast<uint32_t>(kCuLdsBytes / (frames_per_cu + 1) + 1024) & ~15u;
    }
}

Engine::~Engine()
{
    for (void *p : owned_)
        (void)hipFree(p);
    for (auto &q : prof_pending_)
        for (void *e : q)
            prof_free_.push_back(e);
    for (void *e : prof_free_)
        if (e)
            (void)hipEventDestroy(static_cast<hipEvent_t>(e));
    for (int i = 0; i < 2; ++i)
    {
        if (ev_pairs_ready_[i])
            (void)hipEventDestroy(static_cast<hipEvent_t>(ev_pairs_ready_[i]));
        if (ev_pairs_free_[i])
            (void)hipEventDestroy(static_cast<hipEvent_t>(ev_pairs_free_[i]));
    }
    if (rng_stream_)
        (void)hipStreamDestroy(static_cast<hipStream_t>(rng_stream_));
    if (pin_in_ev_)
        (void)hipEventDestroy(static_cast<hipEvent_t>(pin_in_ev_));
}

void Engine::set_profiling(bool on) { profiling_ = on; }

// Every public entry point binds the calling thread to this engine's GPU: the current device is per-thread state, and
// a context used from a new thread (or after another engine switched devices) would otherwise launch on device 0 with
// this device's pointers.
void Engine::bind_device()
{
    if (!device_checked_)
    {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= device_)
        {
            (void)hipGetLastError();
            throw std::runtime_error("no usable HIP device (MI355X required): " + std::string(hipGetErrorString(e)));
        }
        device_checked_ = true;
    }
    check(hipSetDevice(device_), "hipSetDevice");
}

// Event pairs are queued per launch and only read back in last_ms(), so that profiling does not serialise
// the noise stream of batch s+1 behind the decode of batch s.
void Engine::prof_mark(int which, void *stream)
{
    if (!profiling_)
        return;
    auto &q = prof_pending_[which];
    if (q.size() >= 8192 && q.size() % 2 == 0) // nobody is reading: keep the queue bounded
    {
        prof_free_.insert(prof_free_.end(), q.begin(), q.end());
        q.clear();
    }
    void *e;
    if (prof_free_.empty())
    {
        hipEvent_t ev;
        check(hipEventCreate(&ev), "hipEventCreate");
        e = ev;
    }
    else
    {
        e = prof_free_.back();
        prof_free_.pop_back();
    }
    check(hipEventRecord(static_cast<hipEvent_t>(e), static_cast<hipStream_t>(stream)), "event");
    q.push_back(e);
}

// mean duration (ms) of the launches of kind `which` (0 decode kernel, 1 noise stream) since the previous call
float Engine::last_ms(int which)
{
    if (which == 2 || which == 3)
    {
        const int k = which - 2;
        const float v = host_n_[k] ? static_cast<float>(host_ms_[k] / static_cast<double>(host_n_[k])) : 0.f;
        host_ms_[k] = 0, host_n_[k] = 0;
        return v;
    }
    bind_device();
    auto &q = prof_pending_[which ? 1 : 0];
    double sum = 0;
    size_t spans = 0;
    for (size_t i = 0; i + 1 < q.size(); i += 2)
    {
        hipEvent_t a = static_cast<hipEvent_t>(q[i]), b = static_cast<hipEvent_t>(q[i + 1]);
        float ms = 0.f;
        if (hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess)
            sum += ms, ++spans;
        else
            (void)hipGetLastError();
    }
    for (void *e : q)
        prof_free_.push_back(e);
    q.clear();
    return spans ? static_cast<float>(sum / spans) : 0.f;
}

// (at least 16 bytes, so that an empty table still has an address a wave may load a descriptor from)
const void *Engine::upload_table(const void *src, size_t bytes, const char *what)
{
    void *d = nullptr;
    check(hipMalloc(&d, std::max<size_t>(bytes, 16)), (std::string("hipMalloc ") + what).c_str());
    owned_.push_back(d);
    if (bytes)
        check(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice), (std::string("upload ") + what).c_str());
    return d;
}

void Engine::upload_plan()
{
    bind_device();
    if (dev_.cn_blocks)
        return;
    const auto up = [&](const void *src, size_t bytes) { return upload_table(src, bytes, "plan"); };
    const Plan &p = plan_;
#define UP(field, vec) dev_.field = static_cast<decltype(dev_.field)>(up(vec.data(), vec.size() * sizeof(vec[0])))
    UP(cn_blocks, p.cn_blocks);
    UP(vn_blocks, p.vn_blocks);
    UP(vn_slot, p.vn_slot);
    UP(cn_work, p.cn_work);
    UP(cn_work_desc, p.cn_work_desc);
    UP(vn_work_desc, p.vn_work_desc);
    if (!p.vn_packed.empty()) // (else it stays null)
        UP(vn_packed, p.vn_packed);
    dev_.cn_desc_stride = p.cn_desc_stride;
    UP(vn_work, p.vn_work);
    UP(col_rank, p.col_rank);
    UP(rank_col, p.rank_col);
    UP(tx_rank, p.tx_rank);
    UP(rank_kind, p.rank_kind);
    UP(rank_slot0, p.rank_slot0);
    UP(bit_pos, code_->bit_pos);
#undef UP
    if (reg_plan_.ok)
    {
        const RegPlan &r = reg_plan_;
        dev_reg_.nt = r.nt, dev_reg_.kc = r.kc, dev_reg_.maxd = r.maxd, dev_reg_.rounds = r.rounds;
        dev_reg_.mb_doubles = r.mb_doubles;
        dev_reg_.cn_edge = static_cast<const uint32_t *>(up(r.cn_edge.data(), r.cn_edge.size() * 4));
        dev_reg_.cn_deg = static_cast<const uint8_t *>(up(r.cn_deg.data(), r.cn_deg.size()));
        dev_reg_.cn_cnt = static_cast<const uint8_t *>(up(r.cn_cnt.data(), r.cn_cnt.size()));
        dev_reg_.vn_blocks = static_cast<const RegVnBlock *>(up(r.vn_blocks.data(), r.vn_blocks.size() * sizeof(RegVnBlock)));
        dev_reg_.round_first = static_cast<const uint32_t *>(up(r.round_first.data(), r.round_first.size() * 4));
    }
    if (reg2_plan_.ok)
    {
        const Reg2Plan &r = reg2_plan_;
        dev_reg2_.nt = r.nt, dev_reg2_.kc = r.kc, dev_reg2_.maxd = r.maxd, dev_reg2_.nv0 = r.nv0, dev_reg2_.nv1 = r.nv1;
        dev_reg2_.neutral = r.neutral, dev_reg2_.lds_entries = r.lds_entries;
        dev_reg2_.uniform_cn = r.uniform_cn ? 1 : 0;
        dev_reg2_.uniform_vn = r.uniform_vn ? 1 : 0;
        std::memcpy(dev_reg2_.vn_affine, r.vn_affine, sizeof r.vn_affine);
        dev_reg2_.edge_w = static_cast<const uint32_t *>(up(r.edge_w.data(), r.edge_w.size() * 4));
        dev_reg2_.cn_deg = static_cast<const uint8_t *>(up(r.cn_deg.data(), r.cn_deg.size()));
        dev_reg2_.vn_blocks = static_cast<const Reg2VnBlock *>(up(r.vn_blocks.data(), r.vn_blocks.size() * sizeof(Reg2VnBlock)));
        dev_reg2_.vn_rank = static_cast<const uint32_t *>(up(r.vn_rank.data(), r.vn_rank.size() * 4));
    }
    if (fused_plan_.ok)
    {
        const FusedPlan &f = fused_plan_;
        dev_fused_.n_slots = f.n_slots, dev_fused_.vnb = f.vnb, dev_fused_.cnl = f.cnl, dev_fused_.calls_stride = f.calls_stride;
        dev_fused_.has_shortened = f.has_shortened ? 1 : 0;
        dev_fused_.need_lambda = f.need_lambda ? 1 : 0;
        dev_fused_.wide_exclusive = f.wide_exclusive ? 1 : 0;
        dev_fused_.program = f.program;
        std::memcpy(dev_fused_.vn_prog, f.vn_prog, sizeof f.vn_prog);
        // the message slots; the prologue stages one 16-byte entry per transmitted bit or column (+ 2) in the same space
        dev_fused_.lds_bytes = static_cast<uint32_t>(std::max<size_t>(8 * static_cast<size_t>(f.n_slots), 16 * (static_cast<size_t>(std::max(p.nc, p.nct)) + 2)) + 15) & ~15u;
        dev_fused_.leaf_calls = static_cast<const FusedCall *>(up(f.leaf_calls.data(), f.leaf_calls.size() * sizeof(FusedCall)));
        dev_fused_.calls = static_cast<const FusedCall *>(up(f.calls.data(), f.calls.size() * sizeof(FusedCall)));
        dev_fused_.vn_desc = static_cast<const uint32_t *>(up(f.vn_desc.data(), f.vn_desc.size() * 4));
        dev_fused_.vn_slot = static_cast<const uint32_t *>(up(f.vn_slot.data(), f.vn_slot.size() * 4));
        dev_fused_.lane_tab = static_cast<const uint32_t *>(up(f.lane_tab.data(), f.lane_tab.size() * 4));
        dev_fused_.ho_map = static_cast<const uint32_t *>(up(f.ho_map.data(), f.ho_map.size() * 4));
    }
    if (code_->has_G())
    {
        std::vector<uint32_t> cp(code_->G.cptr.begin(), code_->G.cptr.end()), cr(code_->G.crow.begin(), code_->G.crow.end());
        g_col_ptr_ = static_cast<const uint32_t *>(up(cp.data(), cp.size() * 4));
        g_col_row_ = static_cast<const uint32_t *>(up(cr.data(), cr.size() * 4));
        const int kc = code_->kc(), words = (kc + 63) / 64;
        if (kc > 0 && words <= 4 && code_->G.rows <= kc)
        {
            std::vector<uint64_t> mask(static_cast<size_t>(p.nc) * words, 0);
            for (int j = 0; j < code_->G.cols && j < p.nc; ++j)
                for (int q = code_->G.cptr[j]; q < code_->G.cptr[j + 1]; ++q)
                {
                    const int r = code_->G.crow[q];
                    mask[static_cast<size_t>(j) * words + r / 64] ^= 1ull << (r % 64); // (a repeated entry cancels, as in the walk)
                }
            g_mask_ = static_cast<const uint64_t *>(up(mask.data(), mask.size() * 8));
        }
    }
    dev_.lds_bytes = static_cast<uint32_t>(p.lds_bytes);
}

void Engine::synchronize(void *stream)
{
    bind_device();
    check(hipStreamSynchronize(static_cast<hipStream_t>(stream)), "sync");
}

// frames per launch: bounded so that the noise-stream buffers and the memory-resident workspace stay modest
uint64_t Engine::max_sub_batch() const
{
    // the normals of a batch: at most kMaxSlabs chunk slabs (4 GB) per buffer
    const uint64_t kMaxSlabs = std::max<uint64_t>(4, 476ull * 2240 / noise_.st.chunk_blocks());
    const uint64_t pairs_per_frame = std::max<uint64_t>(1, (static_cast<uint64_t>(plan_.nct) + 1) / 2 + 1);
    const uint64_t by_noise = std::max<uint64_t>(1, (kMaxSlabs - 2) * noise_.st.chunk_trials() * 3 / 4 / pairs_per_frame);
    if (residency_ == Residency::kLds || register_resident())
        return std::min<uint64_t>(1u << 17, by_noise);
    const uint64_t per_frame = 8ull * plan_.nnz + 8ull * plan_.nc + plan_.nnz;
    return std::max<uint64_t>(1, std::min<uint64_t>({1u << 17, (8ull << 30) / per_frame, by_noise}));
}

// The host plans of the opt-in variants: built at the first question (a setter, an LDS figure, a launch, the self-test), kept
const LayerPlan &Engine::layer_plan()
{
    return layer_plan_ ? *layer_plan_ : (++layer_plan_builds_, layer_plan_.emplace(build_layer_plan(*code_, plan_)));
}
const QmsPlan &Engine::qms_plan() { return qms_plan_ ? *qms_plan_ : qms_plan_.emplace(build_qms_plan(*code_, plan_)); }

// LDS of one frame of layered sum-product (kernels_layered.hip): binary32 totals and messages of msg_bytes each, or the 8 nc
// bytes the channel writes first
static size_t layered_region_bytes(const LayerPlan &L, size_t nc, size_t msg_bytes)
{
    return (std::max(8 * nc, 4 * ((nc + 3) & ~size_t(3)) + msg_bytes * L.slots) + 15) & ~size_t(15);
}

int64_t Engine::lds_bytes(Decoder d)
{
    const Plan &p = plan_;
    const size_t nc = static_cast<size_t>(p.nc);
    switch (d)
    {
    case Decoder::kLayeredMinSum:
    case Decoder::kLayeredFixedMinSum:
    {
        const LayerPlan &L = layer_plan();
        if (!L.ok || p.has_isolated_vn)
            return -1;
        if (d == Decoder::kLayeredMinSum)
            return static_cast<int64_t>(layered_ms_region_bytes(L, nc));
        return p.nc > 0xFFFF ? -1 : static_cast<int64_t>(layered_fixed_region_bytes(layered_ms_records(L) / 20, nc));
    }
    case Decoder::kQuantizedMinSum:
        return qms_plan().ok ? static_cast<int64_t>(qms_region_bytes(qms_plan().slots, nc)) : -1;
    case Decoder::kTernary:
        // the general plan is all it needs.  A u16 holds a slot and a rank, a wave's work list the lanes of a register (blocks
        // / 8 <= 64), seven planes a column's total (degree + 7 <= 63), the message words the error count's (kernels_ternary.hip)
        if (p.nc > 0xFFFF || p.nnz <= 0 || p.nnz > 0xFFFF || p.max_vn_degree > kTernaryMaxVnDegree || p.cn_blocks.size() > 512 ||
            p.vn_blocks.size() > 512 || static_cast<size_t>(p.n_bitpos) > ternary_message_words(p.nnz, p.nc))
            return -1;
        return static_cast<int64_t>(ternary_lds_bytes(p.nnz, p.nc, ternary_planes(p.max_vn_degree), true));
    default: // the resident decoders and the sum-product modes have no figure of this kind
        return -1;
    }
}

int64_t Engine::layered_fixed_direct_lds_bytes()
{
    const LayerPlan &L = layer_plan();
    return !L.ok || plan_.has_isolated_vn || plan_.nc > 0xFFFF
               ? -1
               : static_cast<int64_t>(layered_fixed_direct_region_bytes(layered_ms_records(L) / 20, static_cast<size_t>(plan_.nc)));
}

// a min-sum variant: its plan takes the code (bytes >= 0, else `outside` says what it takes) and `unit` fits the LDS of a CU
static std::string lds_refusal(int64_t bytes, const std::string &outside, const char *unit)
{
    if (bytes < 0)
        return outside;
    if (bytes > static_cast<int64_t>(kCuLdsBytes))
        return std::string(unit) + " take " + std::to_string(bytes) + " bytes of LDS, more than " + std::to_string(kCuLdsBytes);
    return "";
}

// What each opt-in variant takes, once (engine.hpp).  The texts are what callers see: the two sum-product modes whole, at
// the first decode; the min-sum ones behind their setter's name, at set time
std::string Engine::refusal(Decoder d)
{
    switch (d)
    {
    case Decoder::kResident:
        break;
    case Decoder::kFast32:
        if (!fast_mode_supported(dev_, plan_.max_cn_degree) || plan_.has_isolated_vn)
            return "fast mode: this code is outside what the binary32 kernel takes (check nodes up to degree 8, "
                   "nc <= 8192, LDS-resident, no isolated variable node)";
        break;
    case Decoder::kLayered32:
    case Decoder::kLayered16:
        if (!layer_plan().ok || plan_.has_isolated_vn ||
            layered_region_bytes(layer_plan(), static_cast<size_t>(plan_.nc), d == Decoder::kLayered16 ? 2 : 4) > kCuLdsBytes)
            return "layered mode: this code is outside what the layered kernel takes (check nodes of degree 2..8, at "
                   "most 65535 columns, totals and messages of one frame within 160 KB of LDS, no isolated variable node)";
        break;
    case Decoder::kLayeredMinSum:
        return lds_refusal(lds_bytes(d),
                           "the layered schedule takes codes whose check nodes all have degree 2..8, with at most 65535 columns and no "
                           "isolated variable node",
                           "a frame's totals and check-node records");
    case Decoder::kQuantizedMinSum:
        return lds_refusal(lds_bytes(d), "quantized min-sum takes codes of at most 65535 columns", "a frame's messages, totals and channel values");
    case Decoder::kLayeredFixedMinSum:
        return lds_refusal(lds_bytes(d),
                           "fixed-point layered min-sum takes codes whose check nodes all have degree 2..8, with at most 65535 columns and "
                           "no isolated variable node",
                           "a frame's channel values, totals and check-node records");
    case Decoder::kTernary:
        return lds_refusal(lds_bytes(d),
                           "ternary min-sum takes codes of at most 65535 columns and 65535 edges with column degrees up to " +
                               std::to_string(kTernaryMaxVnDegree) + " (and at most 512 blocks of 64 equal-degree nodes on either side)",
                           "a group's messages, decisions and totals (32 frames)");
    }
    return "";
}

// What the four setters share, once each has checked its own arguments: at most one variant is in force, on a code its
// decoder takes.  Throws behind the setter's name and changes nothing, or puts v in force
void Engine::enter_ms_variant(MsVariant v)
{
    const std::string who = std::string(ms_info(v).setter) + ": ";
    if (ms_variant_ != v && ms_variant_ != MsVariant::kFlooding)
    {
        // (fixed-point layered min-sum tells the other layered decoder from itself)
        const bool two_layered = v == MsVariant::kLayeredFixed && ms_variant_ == MsVariant::kLayered;
        throw std::runtime_error(who + ms_info(v).subject + " does not combine with " +
                                 (two_layered ? "the (binary64) layered schedule" : ms_info(ms_variant_).obstacle) + " (" +
                                 ms_info(ms_variant_).off_first + " first)");
    }
    if (const std::string why = refusal(ms_info(v).decoder); !why.empty())
        throw std::runtime_error(who + why);
    ms_variant_ = v;
}

void Engine::set_ms_schedule(int schedule)
{
    if (schedule != 0 && schedule != 1)
        throw std::runtime_error(std::string(ms_info(MsVariant::kLayered).setter) + ": unknown schedule " + std::to_string(schedule) +
                                 " (0 = flooding, 1 = layered)");
    if (schedule == 0)
        return leave_ms_variant(MsVariant::kLayered);
    enter_ms_variant(MsVariant::kLayered);
}

void Engine::set_ms_quantization(int bits, double step)
{
    if (bits == 0) // off: the step is ignored
        return leave_ms_variant(MsVariant::kQuantized);
    // (the comparisons are false for NaN: a NaN fails them)
    if (bits < 2 || bits > 8 || !(step >= 0x1p-20 && step <= 0x1p20))
        throw std::runtime_error(std::string(ms_info(MsVariant::kQuantized).setter) +
                                 ": need bits 0 (off) or 2..8 and 2^-20 <= step <= 2^20, got (" + std::to_string(bits) + ", " +
                                 std::to_string(step) + ")");
    enter_ms_variant(MsVariant::kQuantized);
    ms_bits_ = bits, ms_step_ = step;
}

void Engine::set_ms_ternary(int weight)
{
    if (weight == 0)
        return leave_ms_variant(MsVariant::kTernary);
    if (weight < 0 || weight > 7)
        throw std::runtime_error(std::string(ms_info(MsVariant::kTernary).setter) + ": need weight 0 (off) or 1..7, got " +
                                 std::to_string(weight));
    enter_ms_variant(MsVariant::kTernary);
    ms_ternary_ = weight;
}

void Engine::set_ms_layered_fixed(int msg_bits, int app_bits, double step)
{
    if (msg_bits == 0) // off: the other arguments are ignored
        return leave_ms_variant(MsVariant::kLayeredFixed);
    // (the comparisons are false for NaN: a NaN fails them)
    if (msg_bits < 2 || msg_bits > 8 || app_bits < msg_bits || app_bits > 16 || !(step >= 0x1p-20 && step <= 0x1p20))
        throw std::runtime_error(std::string(ms_info(MsVariant::kLayeredFixed).setter) +
                                 ": need msg_bits 0 (off) or 2..8, msg_bits <= app_bits <= 16 and 2^-20 <= step <= 2^20, got (" +
                                 std::to_string(msg_bits) + ", " + std::to_string(app_bits) + ", " + std::to_string(step) + ")");
    enter_ms_variant(MsVariant::kLayeredFixed);
    ms_lf_msg_bits_ = msg_bits, ms_lf_app_bits_ = app_bits, ms_lf_step_ = step;
}

// The tables of the layered schedule, as kernels_layered.hip and kernels_layered_ms.hip read them (a code refusal() passed)
void Engine::upload_layer_plan()
{
    if (dev_layer_.rec_off)
        return;
    const LayerPlan &L = layer_plan();
    const size_t nc = plan_.nc;
    std::vector<uint32_t> steps;
    for (const LayerStep &l : L.steps)
        steps.push_back(l.off), steps.push_back(static_cast<uint32_t>(l.count) | static_cast<uint32_t>(l.degree) << 16);
    // the steps' neighbour tables as the kernel fetches them: four words per lane, two VN ranks per word
    std::vector<uint32_t> vn4(L.steps.size() * 4 * kWaveSize, 0);
    for (size_t si = 0; si < L.steps.size(); ++si)
        for (int j = 0; j < L.steps[si].degree; ++j)
            for (int l = 0; l < kWaveSize; ++l)
                vn4[(si * 4 + j / 2) * kWaveSize + l] |=
                    static_cast<uint32_t>(L.vn[L.steps[si].off + static_cast<size_t>(j) * kWaveSize + l]) << (16 * (j & 1));
    // layered min-sum: where each step's records sit behind the totals
    std::vector<uint32_t> rec_off;
    dev_layer_.record_bytes = static_cast<uint32_t>(layered_ms_records(L, &rec_off));
    dev_layer_.region_bytes_ms = static_cast<uint32_t>(layered_ms_region_bytes(L, nc));
    dev_layer_.n_steps = static_cast<uint32_t>(L.steps.size());
    dev_layer_.slots = L.slots;
    dev_layer_.region_bytes = static_cast<uint32_t>(layered_region_bytes(L, nc, 4));
    dev_layer_.region_bytes_half = static_cast<uint32_t>(layered_region_bytes(L, nc, 2));
    dev_layer_.steps = static_cast<const uint32_t *>(upload_table(steps.data(), steps.size() * 4, "layer plan"));
    dev_layer_.vn4 = static_cast<const uint32_t *>(upload_table(vn4.data(), vn4.size() * 4, "layer plan"));
    dev_layer_.rec_off = static_cast<const uint32_t *>(upload_table(rec_off.data(), rec_off.size() * 4, "layer plan")); // last: the mark
}

// the tables of quantized min-sum (a code refusal() passed)
void Engine::upload_qms_plan()
{
    if (dev_qms_.cn_desc)
        return;
    const QmsPlan &q = qms_plan();
    const char *what = "quantized min-sum plan";
    dev_qms_.cn_vn = static_cast<const uint16_t *>(upload_table(q.cn_vn.data(), 2 * q.cn_vn.size(), what));
    dev_qms_.vn_start = static_cast<const uint32_t *>(upload_table(q.vn_start.data(), 4 * q.vn_start.size(), what));
    dev_qms_.vn_slot = static_cast<const uint32_t *>(upload_table(q.vn_slot.data(), 4 * q.vn_slot.size(), what));
    dev_qms_.slots = q.slots;
    dev_qms_.work_bytes = static_cast<uint32_t>(qms_work_bytes(q.slots, static_cast<size_t>(plan_.nc)));
    dev_qms_.region_bytes = static_cast<uint32_t>(qms_region_bytes(q.slots, static_cast<size_t>(plan_.nc)));
    dev_qms_.cn_desc = static_cast<const uint32_t *>(upload_table(q.cn_desc.data(), 4 * q.cn_desc.size(), what)); // last: the mark
}

// The correction table of the two fixed-point min-sum modes (include/ldpc_amd.h, ldpc_hip_set_min_sum_quantization, item 3):
// lut[m], m = 0..qmax, four per word; binary64, every operation rounded once (-ffp-contract=off), rint = round-half-to-even
static void correction_lut(double scale, double offset, double inv, int qmax, uint32_t (&lut)[32])
{
    const double off = offset * inv;
    for (int m = 0; m <= qmax; ++m)
    {
        const double t = scale * static_cast<double>(m);
        const double r = std::rint(t - off); // (scale <= 1 and off >= 0: never above m)
        const uint32_t v = r > 0.0 ? static_cast<uint32_t>(r) : 0u;
        lut[m >> 2] |= v << (8 * (m & 3));
    }
}

// the quantizer (item 1: the step and fl(1 / step), computed here), the largest message magnitude and the correction table
// of one launch: what the arguments of the two fixed-point modes share (ldpc_hip_set_min_sum_layered_fixed, items 1 and 3)
template <class Args>
static Args quantizer_args(double step, int msg_bits, double scale, double offset)
{
    Args q{};
    q.step = step, q.inv = 1.0 / step;
    q.qmax = (1 << (msg_bits - 1)) - 1;
    correction_lut(scale, offset, q.inv, q.qmax, q.lut);
    return q;
}

QmsArgs Engine::qms_args() const { return quantizer_args<QmsArgs>(ms_step_, ms_bits_, ms_scale, ms_offset); }

LayeredFixedArgs Engine::layered_fixed_args() const
{
    LayeredFixedArgs q = quantizer_args<LayeredFixedArgs>(ms_lf_step_, ms_lf_msg_bits_, ms_scale, ms_offset);
    q.pmax = (1 << (ms_lf_app_bits_ - 1)) - 1;
    return q;
}

void Engine::finish_batch(OutStage &st, const BatchOut &out, uint64_t n, const uint8_t *codeword, int noise_buffer, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nc = plan_.nc;
    prof_mark(0, s);
    if (noise_buffer >= 0)
        noise_raw_release(noise_buffer, stream);
    if (out.codeword)
    {
        if (codeword)
            check(hipMemcpyAsync(out.codeword, codeword, n * nc,
                                 is_device_ptr(out.codeword) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s),
                  "codeword out");
        else if (is_device_ptr(out.codeword))
            check(hipMemsetAsync(out.codeword, 0, n * nc, s), "codeword out");
        else
            std::memset(out.codeword, 0, n * nc);
    }
    st.flush(s, &pin_out_);
}

// the list pointers a stage reads (`in`) and writes (`out`): buffers of [count][n frames][n resume iterations]
static void set_stage_lists(DecodeArgs &a, Stage st, uint32_t *in, uint32_t *out, uint64_t n)
{
    const bool reads = stage_reads_list(st), writes = stage_writes_list(st);
    a.redo_count_in = reads ? in : nullptr, a.redo_list_in = reads ? in + 1 : nullptr;
    a.redo_iter_in = st == Stage::kHandoverResume ? in + 1 + n : nullptr;
    a.redo_count = writes ? out : nullptr, a.redo_list = writes ? out + 1 : nullptr;
    a.redo_iter = st == Stage::kHandoverFirst ? out + 1 + n : nullptr;
}

void Engine::run_decode(DecodeArgs &a, const DecParams &p, const BatchOut &out, uint64_t n, void *stream, const TypedIo *typed)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nc = plan_.nc, nnz = plan_.nnz;
    // the caller's opt-in variant, or the resident decoder; a variant that does not take the code launches nothing
    const Decoder dec = decoder(p);
    if (const std::string why = refusal(dec); !why.empty())
        throw std::runtime_error(why);
    OutStage st;
    a.plan = dev_;
    a.iterations = p.iterations;
    a.early_term = p.early_term;
    a.n_frames = n;
    a.iters = st.route(out.iters, stage_iters_, 4 * n);
    a.bit_errors = st.route(out.bit_errors, stage_be_, 4 * n);
    a.hard = st.route(out.hard, stage_hard_, n * nc);
    a.llr_out = st.route(out.llr_out, stage_llr_out_, 8 * n * nc);
    a.llr_in_dump = st.route(out.llr_in, stage_llr_in_, 8 * n * nc);
    // typed batch call: the packed decisions come from the decision bytes, the staged ones where the caller wants none
    uint32_t *const hard_bits = typed ? st.route(typed->hard_bits, stage_bits_, 4 * n * ((nc + 31) / 32)) : nullptr;
    if (hard_bits && !a.hard)
        a.hard = static_cast<uint8_t *>(stage_hard_.reserve(n * nc));
    const auto pack = [&] {
        if (hard_bits)
            check(launch_pack_hard(a.hard, n, plan_.nc, hard_bits, s), "pack decisions");
    };
    // ... and its input: fixed-point layered min-sum reads it as it is, every other decoder its binary64 image
    const bool direct = typed && typed->llr && dec == Decoder::kLayeredFixedMinSum;
    // (1, 0) is plain min-sum: the launches of today, not corrected instantiations that would compute the same
    a.ms_correct = p.min_sum && !(ms_scale == 1.0 && ms_offset == 0.0);
    a.ms_scale = ms_scale, a.ms_offset = ms_offset;
    prof_mark(0, s);
    if (typed && typed->llr && !direct)
    {
        double *w = static_cast<double *>(stage_in_.reserve(8 * n * nc));
        check(launch_widen_llr(typed->llr, typed->type, typed->step, n * nc, w, s), "widen typed LLRs");
        a.llr_in = w;
    }
    const auto launch = [&](Stage stage) {
        switch (dec)
        {
        case Decoder::kLayeredMinSum:
            upload_layer_plan();
            check(launch_decode_layered_ms(a, dev_layer_, s), "decode (layered min-sum)");
            return;
        case Decoder::kQuantizedMinSum:
            upload_qms_plan();
            check(launch_decode_qms(a, dev_qms_, qms_args(), s), "decode (quantized min-sum)");
            return;
        case Decoder::kLayeredFixedMinSum:
            upload_layer_plan();
            if (direct)
                check(launch_decode_layered_fixed_direct(a, dev_layer_, layered_fixed_args(), TypedLlrArgs{typed->llr, typed->type, 0}, s),
                      "decode (fixed-point layered min-sum, typed LLRs)");
            else
                check(launch_decode_layered_fixed(a, dev_layer_, layered_fixed_args(), s), "decode (fixed-point layered min-sum)");
            return;
        case Decoder::kTernary:
            check(launch_decode_ternary(a, TernaryArgs{ms_ternary_, ternary_planes(plan_.max_vn_degree)}, s), "decode (ternary min-sum)");
            return;
        case Decoder::kFast32:
            a.ws_hb = static_cast<uint8_t *>(ws_hb_.reserve(n * nc));
            check(launch_decode_fast(a, plan_.max_cn_degree, s), "decode (fast mode, binary32)");
            return;
        case Decoder::kLayered32:
        case Decoder::kLayered16:
            upload_layer_plan();
            check(launch_decode_layered(a, dev_layer_, dec == Decoder::kLayered16, s),
                  dec == Decoder::kLayered16 ? "decode (layered, binary16 messages)" : "decode (layered, binary32 messages)");
            return;
        case Decoder::kResident:
            break;
        }
        switch (residency_)
        {
        case Residency::kLds:
            // codes the fused form takes (fused_rule.h): the first launch of sum-product — without early termination with
            // separately divided outputs, its messages handed over as LLRs — and min-sum without early termination
            if (fused_plan_.ok && stage == Stage::kRatioFirst)
                check(launch_decode_fused(a, dev_fused_, stage, s), "decode (fused form)");
            else if (fused_plan_.ok && stage == Stage::kHandoverFirst)
                check(launch_decode_fused(a, dev_fused_, stage, s), "decode (fused form, hand-over)");
            else if (fused_plan_.ok && stage == Stage::kWhole && p.min_sum && !p.early_term && p.iterations > 0)
                check(launch_decode_fused(a, dev_fused_, stage, s), "decode (min-sum, fused plan)");
            else
                check(launch_decode_lds(a, stage, p.min_sum, plan_.max_cn_degree, lds_llr_mode_, s), "decode (LDS-resident)");
            break;
        case Residency::kRegTotals:
        case Residency::kRegMessages:
            a.ws_llr = static_cast<double *>(ws_llr_.reserve(8 * n * nc));
            a.ws_hb = static_cast<uint8_t *>(ws_hb_.reserve(n * nc));
            if (residency_ == Residency::kRegTotals)
            {
                // channel terms of the variable nodes, one per (block slot, thread): kernels_reg2.hip
                a.ws_scr = static_cast<double *>(ws_scr_.reserve(8 * n * static_cast<uint64_t>(reg2_plan_.nv0 + reg2_plan_.nv1) * reg2_plan_.nt));
                check(launch_decode_reg2(a, dev_reg2_, stage, p.min_sum, s), "decode (register-resident, totals form)");
            }
            else
                check(launch_decode_reg(a, dev_reg_, stage, p.min_sum, s), "decode (register-resident)");
            break;
        case Residency::kMemory:
            a.ws_msg = static_cast<double *>(ws_msg_.reserve(8 * n * nnz));
            a.ws_llr = static_cast<double *>(ws_llr_.reserve(8 * n * nc));
            a.ws_hb = static_cast<uint8_t *>(ws_hb_.reserve(n * nnz));
            a.ws_scr = plan_.max_cn_degree > kMaxCnDegree ? static_cast<double *>(ws_scr_.reserve(16 * n * nnz)) : nullptr;
            check(launch_decode_mem(a, stage, p.min_sum, plan_.max_cn_degree, mem_occ_lds_, s), "decode (memory-resident)");
            break;
        case Residency::kNone:
            throw std::runtime_error("code not supported by any decoder instantiation");
        }
    };
    const StageSeq seq = stages(p);
    uint32_t *list_in = nullptr; // what the stage before handed on
    for (int i = 0; i < seq.n; ++i)
    {
        const Stage stage = seq.s[i];
        uint32_t *list_out = nullptr;
        if (stage_writes_list(stage))
        {
            list_out = static_cast<uint32_t *>(i == 0 ? redo_.reserve(4 * (2 * n + 1)) : redo2_.reserve(4 * (n + 1)));
            check(hipMemsetAsync(list_out, 0, 4, s), "redo count");
        }
        set_stage_lists(a, stage, list_in, list_out, n);
        if (stage == Stage::kHandoverFirst)
            a.ws_handover = static_cast<double *>(ws_msg_.reserve(8 * n * nnz));
        if (stage == Stage::kHandoverResume) // (the fused form hands its messages over as LLRs)
            a.handover_llr = fused_plan_.ok ? 1 : 0;
#ifdef LDPC_AMD_PHASE_TRACE
        uint64_t *tr = nullptr;
        // debug build: per-wave phase timers of the first 2048 frames
        const char *trace_file = i == 0 && stage != Stage::kWhole ? std::getenv("LDPC_AMD_PHASE_TRACE") : nullptr;
        if (trace_file)
        {
            check(hipMalloc(&tr, 2048 * 32 * 8), "trace");
            check(hipMemset(tr, 0, 2048 * 32 * 8), "trace");
            a.phase_trace = tr;
        }
#endif
        launch(stage);
#ifdef LDPC_AMD_PHASE_TRACE
        if (tr)
        {
            std::vector<uint64_t> h(2048 * 32);
            check(hipDeviceSynchronize(), "sync");
            check(hipMemcpy(h.data(), tr, 2048 * 32 * 8, hipMemcpyDeviceToHost), "trace");
            if (FILE *f = std::fopen(trace_file, "wb"))
            {
                std::fwrite(h.data(), 8, h.size(), f);
                std::fclose(f);
            }
            (void)hipFree(tr);
            a.phase_trace = nullptr;
        }
#endif
        // A handful of frames for a caller who waits for host results anyway (the reference's decode(): one frame per call):
        // the results of the first launch and the number of frames it handed back travel to the host together; the later
        // launches — two more dispatches and a memset, a fifth of such a call's latency, for lists that are almost always
        // empty — are issued only when that number is not zero, and the results delivered again.
        const size_t pinned = st.pinned_bytes();
        const bool deliver_now = i == 0 && stage == Stage::kRatioFirst && n <= 16 && pinned && pinned <= OutStage::kPinnedLimit && a.mode == kModeLlr;
        if (deliver_now)
            pack(); // (of this launch's decisions: they travel now)
        if (deliver_now && st.flush(s, &pin_out_, list_out) == 0)
        {
            st.items.clear(); // (delivered)
            break;
        }
        list_in = list_out;
    }
    set_stage_lists(a, Stage::kWhole, nullptr, nullptr, n);
    a.ws_handover = nullptr, a.handover_llr = 0;
    pack();
    finish_batch(st, out, n, a.codeword, a.mode == kModeAwgn ? a.pairs_buffer : -1, stream);
}

void Engine::run_bsc(DecodeArgs &a, const DecParams &p, const BatchOut &out, uint64_t n, uint64_t raw_first, void *stream)
{
    a.mode = kModeBsc;
    int raw_buffer = 0;
    a.raw = noise_raw_async(raw_first, n * static_cast<uint64_t>(plan_.nct), stream, raw_buffer);
    a.eps = x_, a.delta = delta_;
    a.shorten_llr = delta_; // channel.cpp:152
    run_decode(a, p, out, n, stream);
    noise_raw_release(raw_buffer, stream);
}

void Engine::run_bec(const DecParams &p, const BatchOut &out, uint64_t n, const uint8_t *codeword, uint64_t raw_first, void *stream,
                     const uint64_t *ctr_frame0)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nc = plan_.nc;
    const uint64_t nct = static_cast<uint64_t>(plan_.nct);
    const size_t state = bec_state_bytes(plan_.nnz, plan_.nc);
    OutStage st;
    BecArgs a{};
    a.ws = state > kCuLdsBytes ? static_cast<uint8_t *>(ws_msg_.reserve(n * state)) : nullptr; // beyond LDS: state in memory
    a.plan = dev_;
    a.iterations = p.iterations;
    a.early_term = p.early_term;
    a.deg1_compat = bec_deg1_compat;
    a.n_frames = n;
    int raw_buffer = -1;
    if (ctr_frame0)
    {
        a.counter = 1;
        a.ctr_key[0] = static_cast<uint32_t>(ctr_seed_), a.ctr_key[1] = static_cast<uint32_t>(ctr_seed_ >> 32);
        a.ctr_frame0 = *ctr_frame0;
    }
    else
        a.raw = noise_raw_async(raw_first, n * nct, stream, raw_buffer);
    a.eps = x_;
    a.codeword = codeword;
    a.iters = st.route(out.iters, stage_iters_, 4 * n);
    a.bit_errors = st.route(out.bit_errors, stage_be_, 4 * n);
    a.hard = st.route(out.hard, stage_hard_, n * nc);
    a.llr_out = st.route(out.llr_out, stage_llr_out_, 8 * n * nc);
    a.llr_in_dump = st.route(out.llr_in, stage_llr_in_, 8 * n * nc);
    prof_mark(0, s);
    check(launch_bec(a, s), "bec");
    finish_batch(st, out, n, codeword, raw_buffer, stream);
}

uint8_t *Engine::encoder_prologue(uint64_t frames_kept, bool sharded, void *stream)
{
    const int kc = code_->kc();
    if (kc <= 0 || code_->G.rows > kc)
        throw std::runtime_error("generator matrix does not match the code (rows > nc - mc)");
    if (sharded && static_cast<size_t>((kc + 63) / 64) * 8 > Comm::kMaxBytes)
        throw std::runtime_error("sharded encoding: more than 2048 information bits per frame do not fit the exchange");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nc = plan_.nc;
    uint8_t *prev = static_cast<uint8_t *>(cw_run_.reserve(nc));
    if (!cw_run_valid_)
    {
        check(hipMemsetAsync(prev, 0, nc, s), "codeword reset");
        cw_run_valid_ = true;
    }
    check(hipMemcpyAsync(cw_before_.reserve(nc), prev, nc, hipMemcpyDeviceToDevice, s), "codeword snapshot");
    last_enc_n_ = frames_kept;
    return prev;
}

// channel.cpp:44-60 for n consecutive frames (see EncodeArgs in kernels.hpp)
const uint8_t *Engine::encode_frames(uint64_t n, bool want_codewords, void *stream)
{
    if (!code_->has_G() || n == 0)
        return nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nc = plan_.nc;
    const uint64_t kc = static_cast<uint64_t>(code_->kc());
    uint8_t *prev = encoder_prologue(want_codewords ? n : 0, false, stream);
    EncodeArgs e{};
    e.nc = static_cast<int>(nc);
    e.kc = static_cast<int>(kc);
    e.words = static_cast<int>((kc + 63) / 64);
    e.g_col_ptr = g_col_ptr_;
    e.g_col_row = g_col_row_;
    e.g_mask = g_mask_;
    e.g_cols = code_->G.cols;
    e.info_raw = info_.generate(info_pos_, n * kc, stream);
    e.prefix = static_cast<uint64_t *>(enc_prefix_.reserve(8 * n * e.words));
    e.cw_prev = prev;
    e.codeword = want_codewords ? static_cast<uint8_t *>(cw_frames_.reserve(n * nc)) : nullptr;
    e.cw_last = static_cast<uint8_t *>(cw_next_.reserve(nc));
    e.n_frames = n;
    check(launch_encode(e, s), "encode");
    check(hipMemcpyAsync(prev, e.cw_last, nc, hipMemcpyDeviceToDevice, s), "codeword carry");
    info_pos_ += n * kc;
    return e.codeword;
}

const uint8_t *Engine::encode_frames_sharded(Comm &comm, uint64_t before, uint64_t n, uint64_t step_frames, void *stream)
{
    if (!code_->has_G() || step_frames == 0)
        return nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nc = plan_.nc;
    const uint64_t kc = static_cast<uint64_t>(code_->kc());
    uint8_t *prev = encoder_prologue(n, true, stream);
    const int words = static_cast<int>((kc + 63) / 64);
    // this rank's frames: info words and their running XOR (the last entry is the XOR over the rank's range)
    uint64_t *base = static_cast<uint64_t *>(enc_base_.reserve(8 * 2 * static_cast<size_t>(words)));
    EncodeArgs e{};
    e.nc = static_cast<int>(nc), e.kc = static_cast<int>(kc), e.words = words;
    e.g_col_ptr = g_col_ptr_, e.g_col_row = g_col_row_, e.g_cols = code_->G.cols;
    e.g_mask = g_mask_;
    e.cw_prev = prev;
    e.cw_last = static_cast<uint8_t *>(cw_next_.reserve(nc));
    std::vector<uint64_t> mine(words, 0), all(static_cast<size_t>(words) * comm.world());
    if (n)
    {
        e.info_raw = info_.generate(info_pos_ + before * kc, n * kc, stream);
        e.prefix = static_cast<uint64_t *>(enc_prefix_.reserve(8 * n * words));
        e.n_frames = n;
        check(launch_encode_prefix(e, s), "encode (info words)");
        check(hipMemcpyAsync(mine.data(), e.prefix + (n - 1) * words, 8 * static_cast<size_t>(words), hipMemcpyDeviceToHost, s), "info sum");
        check(hipStreamSynchronize(s), "sync");
    }
    // ONE exchange: every rank's sum; the ranks before this one give the word every prefix of this rank starts from, all of
    // them together the codeword after the step (the codeword accumulates linearly: channel.cpp:44-60)
    const auto t0 = std::chrono::steady_clock::now();
    comm.all_gather(mine.data(), all.data(), 8 * static_cast<size_t>(words));
    host_ms_[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::vector<uint64_t> host(2 * static_cast<size_t>(words), 0); // [0, words): ranks before this one; [words, 2 words): all
    for (int q = 0; q < comm.world(); ++q)
        for (int w = 0; w < words; ++w)
        {
            if (q < comm.rank())
                host[w] ^= all[static_cast<size_t>(q) * words + w];
            host[words + w] ^= all[static_cast<size_t>(q) * words + w];
        }
    check(hipMemcpyAsync(base, host.data(), 8 * host.size(), hipMemcpyHostToDevice, s), "info sums");
    check(hipStreamSynchronize(s), "sync"); // (host is a local: the copy must have read it)
    const uint8_t *cw = nullptr;
    if (n)
    {
        e.base = base;
        e.codeword = static_cast<uint8_t *>(cw_frames_.reserve(n * nc));
        check(launch_encode_codewords(e, s, false), "encode (codewords)");
        cw = e.codeword;
    }
    // the codeword after the step, on every rank: cw_prev ^ (sum over all ranks) G — one pseudo-frame whose prefix is that sum
    e.prefix = base + words, e.base = nullptr, e.n_frames = 1, e.codeword = nullptr;
    check(launch_encode_codewords(e, s, true), "encode (codeword carry)");
    check(hipMemcpyAsync(prev, e.cw_last, nc, hipMemcpyDeviceToDevice, s), "codeword carry");
    info_pos_ += step_frames * kc;
    return cw;
}

const uint8_t *Engine::encode_frames_counter(uint64_t frame0, uint64_t n, void *stream)
{
    if (!code_->has_G() || n == 0)
        return nullptr;
    const int kc = code_->kc();
    if (kc <= 0 || code_->G.rows > kc)
        throw std::runtime_error("generator matrix does not match the code (rows > nc - mc)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nc = plan_.nc;
    EncodeArgs e{};
    e.nc = static_cast<int>(nc);
    e.kc = kc;
    e.words = (kc + 63) / 64;
    e.g_col_ptr = g_col_ptr_;
    e.g_col_row = g_col_row_;
    e.g_mask = g_mask_;
    e.g_cols = code_->G.cols;
    // the info words of the frames are the "prefixes" of the codeword launch, joined to an all-zero running codeword: u_f G
    e.prefix = static_cast<uint64_t *>(enc_prefix_.reserve(8 * n * e.words));
    check(launch_encode_info_counter(ctr_seed_, frame0, n, kc, e.words, e.prefix, s), "encode (counter info words)");
    if (!cw_zero_.get() || cw_zero_.size() < nc)
        check(hipMemsetAsync(cw_zero_.reserve(nc), 0, nc, s), "codeword zero");
    e.cw_prev = static_cast<const uint8_t *>(cw_zero_.get());
    e.codeword = static_cast<uint8_t *>(cw_frames_.reserve(n * nc));
    e.cw_last = static_cast<uint8_t *>(cw_next_.reserve(nc));
    e.n_frames = n;
    check(launch_encode_codewords(e, s, false), "encode (counter codewords)");
    return e.codeword;
}

void Engine::run_counter(const DecParams &p, const BatchOut &out, uint64_t frame0, uint64_t n, void *stream)
{
    if (fast_mode)
        throw std::runtime_error("counter-based noise does not combine with the non-parity fast modes (set_fast_mode(0) first)");
    const uint8_t *cw = encode_frames_counter(frame0, n, stream);
    if (chan_ == kBec)
    {
        run_bec(p, out, n, cw, 0, stream, &frame0);
        return;
    }
    DecodeArgs a{};
    a.codeword = cw;
    a.ctr_key[0] = static_cast<uint32_t>(ctr_seed_), a.ctr_key[1] = static_cast<uint32_t>(ctr_seed_ >> 32);
    a.ctr_frame0 = frame0;
    if (chan_ == kAwgn)
    {
        a.mode = kModeAwgnCtr;
        a.sigma = sigma_, a.sigma2 = sigma2_, a.inv_sigma2 = 1.0 / sigma2_;
        a.shorten_llr = 99999.9; // channel.cpp:83
    }
    else
    {
        a.mode = kModeBscCtr;
        a.eps = x_, a.delta = delta_;
        a.shorten_llr = delta_; // channel.cpp:152
    }
    run_decode(a, p, out, n, stream);
}

void Engine::decode_llr(const DecParams &p, uint64_t n, const double *llr_in, const BatchOut &out, void *stream)
{
    decode_typed(p, n, llr_in, kLlrF64, out, nullptr, stream);
}

// int8 LLRs are multiples of a fixed-point mode's step: they need "BP_MS" with quantized or fixed-point layered min-sum on
std::string Engine::typed_refusal(const DecParams &p, int type) const
{
    const std::string who = "ldpc_hip_decode_batch_typed: ";
    if (llr_type_bytes(type) == 0)
        return who + "unknown LLR type " + std::to_string(type) + " (0 = binary64, 1 = binary32, 2 = binary16, 3 = int8)";
    const Decoder d = decoder(p);
    if (type == kLlrI8 && d != Decoder::kQuantizedMinSum && d != Decoder::kLayeredFixedMinSum)
        return who + "int8 LLRs count steps of a fixed-point mode: they need \"BP_MS\" decoding with "
                     "ldpc_hip_set_min_sum_quantization or ldpc_hip_set_min_sum_layered_fixed on";
    return "";
}

void Engine::decode_typed(const DecParams &p, uint64_t n, const void *llr_in, int type, const BatchOut &out, uint32_t *hard_bits, void *stream)
{
    if (const std::string why = typed_refusal(p, type); !why.empty())
        throw std::runtime_error(why);
    if (n == 0)
        return;
    upload_plan();
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), sub = max_sub_batch();
    const size_t elem = llr_type_bytes(type); // the typed source advances in units of its own element size
    const uint64_t words = (nc + 31) / 32;    // ... and the packed decisions in words per frame
    TypedIo io;
    io.type = type;
    switch (ms_variant_) // the step an int8 counts: the fixed-point variant's in force (typed_refusal takes int8 for those alone)
    {
    case MsVariant::kQuantized:
        io.step = ms_step_;
        break;
    case MsVariant::kLayeredFixed:
        io.step = ms_lf_step_;
        break;
    case MsVariant::kFlooding:
    case MsVariant::kLayered:
    case MsVariant::kTernary:
        break;
    }
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        const size_t bytes = elem * m * nc;
        DecodeArgs a{};
        a.mode = kModeLlr;
        // host input is staged in its own type (binary64 where the decoder reads it; the widened image of the others goes there)
        const void *src = stage_input(static_cast<const char *>(llr_in) + elem * done * nc, bytes, type == kLlrF64 ? stage_in_ : stage_typed_, stream);
        if (type == kLlrF64)
            a.llr_in = static_cast<const double *>(src);
        else
            io.llr = src;
        io.hard_bits = hard_bits ? hard_bits + done * words : nullptr;
        run_decode(a, p, out.at(done, nc), m, stream, type == kLlrF64 && !hard_bits ? nullptr : &io);
    }
}

const void *Engine::stage_input(const void *src, size_t bytes, DeviceBuffer &stage, void *stream)
{
    if (is_device_ptr(src))
        return src;
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *d = stage.reserve(bytes);
    const void *from = src;
    if (bytes <= (1u << 20)) // small inputs through page-locked memory (see OutStage::flush)
    {
        if (!pin_in_ev_)
        {
            hipEvent_t ev;
            check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
            pin_in_ev_ = ev;
        }
        else
            check(hipEventSynchronize(static_cast<hipEvent_t>(pin_in_ev_)), "event"); // the previous copy out of the buffer is done
        void *h = pin_in_.reserve(bytes);
        std::memcpy(h, src, bytes);
        from = h;
    }
    check(hipMemcpyAsync(d, from, bytes, hipMemcpyHostToDevice, s), "copy in");
    if (from != src)
        check(hipEventRecord(static_cast<hipEvent_t>(pin_in_ev_), s), "event");
    return d;
}

// ---------------------------------------------------------------------------------------------
// Frames of bits on the device: encode, syndrome, bit errors (kernels_gf2.hip)
static std::string bits_format_refusal(const char *entry, const char *operand, int format)
{
    if (bits_format_known(format))
        return "";
    return std::string(entry) + ": unknown format " + std::to_string(format) + " of " + operand + " (0 = LDPC_HIP_BITS_U8, 1 = LDPC_HIP_BITS_PACKED32)";
}

std::string Engine::encode_refusal(int info_format) const
{
    const char *who = "ldpc_hip_encode_batch";
    if (std::string why = bits_format_refusal(who, "info", info_format); !why.empty())
        return why;
    if (!code_->has_G())
        return std::string(who) + ": the context has no generator matrix";
    const int kc = code_->kc();
    if (kc <= 0 || code_->G.rows > kc)
        return std::string(who) + ": generator matrix does not match the code (rows > nc - mc)";
    if (static_cast<uint64_t>(plan_.nc) * ((static_cast<uint64_t>(kc) + 31) / 32) * 4 > (256ull << 20))
        return std::string(who) + ": the column masks of G (nc x ceil(kc / 32) words) would exceed 256 MiB";
    return "";
}

std::string Engine::syndrome_refusal(int word_format) const
{
    const char *who = "ldpc_hip_syndrome_batch";
    if (std::string why = bits_format_refusal(who, "word", word_format); !why.empty())
        return why;
    const uint32_t nc = static_cast<uint32_t>(plan_.nc);
    if ((256 / (64 * gf2_syndrome_waves_per_frame(nc))) * gf2_syndrome_frame_lds_bytes(nc) > kGf2SyndromeMaxLds)
        return std::string(who) + ": a frame of more than 524 288 columns does not fit the kernel's LDS";
    return "";
}

std::string Engine::bit_errors_refusal(int a_format, int b_format) const
{
    const char *who = "ldpc_hip_bit_errors_batch";
    if (std::string why = bits_format_refusal(who, "a", a_format); !why.empty())
        return why;
    return bits_format_refusal(who, "b", b_format);
}

uint64_t Engine::gf2_sub_batch() const
{
    return std::clamp<uint64_t>((256ull << 20) / static_cast<uint64_t>(plan_.nc), 1, 1u << 20);
}

void Engine::encode_batch(uint64_t n, const void *info, int info_format, uint8_t *codeword, uint32_t *codeword_bits, void *stream)
{
    const char *who = "ldpc_hip_encode_batch";
    if (const std::string why = encode_refusal(info_format); !why.empty())
        throw std::runtime_error(why);
    if (n && !info)
        throw std::runtime_error(std::string(who) + ": null info");
    if (n == 0 || (!codeword && !codeword_bits))
        return;
    bind_device();
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), kc = static_cast<uint64_t>(code_->kc());
    const uint64_t words = (kc + 31) / 32, out_words = (nc + 31) / 32;
    if (!gf2_mask_) // the columns of G as masks over the information word, once per context
    {
        const uint64_t cols = (nc + 255) / 256 * 256;
        std::vector<uint32_t> mask(words * cols, 0);
        const SparseGF2 &G = code_->G;
        for (int j = 0; j < G.cols && static_cast<uint64_t>(j) < nc; ++j)
            for (int q = G.cptr[j]; q < G.cptr[j + 1]; ++q)
            {
                const uint64_t r = static_cast<uint64_t>(G.crow[q]);
                mask[(r / 32) * cols + j] ^= 1u << (r % 32); // (a repeated entry cancels)
            }
        gf2_mask_cols_ = cols;
        gf2_mask_ = static_cast<const uint32_t *>(upload_table(mask.data(), mask.size() * 4, "generator masks"));
    }
    const uint64_t sub = gf2_sub_batch();
    const size_t in_row = bits_row_bytes(info_format, kc);
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        const void *src = stage_input(static_cast<const char *>(info) + in_row * done, in_row * m, stage_in_, stream);
        if (info_format == kBitsU8) // bytes: packed by one small launch in front
        {
            uint32_t *packed = static_cast<uint32_t *>(gf2_info_.reserve(4 * m * words));
            check(launch_pack_hard(static_cast<const uint8_t *>(src), m, static_cast<int>(kc), packed, s), "encode_batch (pack)");
            src = packed;
        }
        OutStage st;
        Gf2EncodeArgs a{};
        a.nc = static_cast<uint32_t>(nc), a.words = static_cast<uint32_t>(words);
        a.mask_cols = gf2_mask_cols_, a.mask = gf2_mask_;
        a.info = static_cast<const uint32_t *>(src);
        a.codeword = st.route(codeword ? codeword + done * nc : nullptr, stage_gf2_[0], m * nc);
        a.codeword_bits = st.route(codeword_bits ? codeword_bits + done * out_words : nullptr, stage_gf2_[1], 4 * m * out_words);
        a.n = m;
        check(launch_gf2_encode(a, s), "encode_batch");
        st.flush(s, &pin_out_);
    }
}

void Engine::upload_rows_of_h()
{
    if (gf2_row_ptr_)
        return;
    const SparseGF2 &H = code_->H;
    std::vector<uint32_t> rp(H.rptr.begin(), H.rptr.end()), rc(H.rcol.begin(), H.rcol.end());
    gf2_row_col_ = static_cast<const uint32_t *>(upload_table(rc.data(), rc.size() * 4, "rows of H"));
    gf2_row_ptr_ = static_cast<const uint32_t *>(upload_table(rp.data(), rp.size() * 4, "rows of H")); // last: the mark
}

void Engine::syndrome_batch(uint64_t n, const void *word, int word_format, uint8_t *syndrome, uint32_t *syndrome_bits, uint32_t *weight,
                            void *stream)
{
    const char *who = "ldpc_hip_syndrome_batch";
    if (const std::string why = syndrome_refusal(word_format); !why.empty())
        throw std::runtime_error(why);
    if (n && !word)
        throw std::runtime_error(std::string(who) + ": null word");
    if (n == 0 || (!syndrome && !syndrome_bits && !weight))
        return;
    bind_device();
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), mc = static_cast<uint64_t>(plan_.mc), out_words = (mc + 31) / 32;
    upload_rows_of_h();
    const uint64_t sub = gf2_sub_batch();
    const size_t in_row = bits_row_bytes(word_format, nc);
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        OutStage st;
        Gf2SyndromeArgs a{};
        a.nc = static_cast<uint32_t>(nc), a.mc = static_cast<uint32_t>(mc);
        a.row_ptr = gf2_row_ptr_, a.row_col = gf2_row_col_;
        a.word = stage_input(static_cast<const char *>(word) + in_row * done, in_row * m, stage_in_, stream);
        a.syndrome = st.route(syndrome ? syndrome + done * mc : nullptr, stage_gf2_[0], m * mc);
        a.syndrome_bits = st.route(syndrome_bits ? syndrome_bits + done * out_words : nullptr, stage_gf2_[1], 4 * m * out_words);
        a.weight = st.route(weight ? weight + done : nullptr, stage_gf2_[2], 4 * m);
        a.n = m;
        check(launch_gf2_syndrome(a, word_format, s), "syndrome_batch");
        st.flush(s, &pin_out_);
    }
}

void Engine::bit_errors_batch(uint64_t n, const void *a_rows, int a_format, const void *b_rows, int b_format, uint32_t *bit_errors,
                              void *stream)
{
    const char *who = "ldpc_hip_bit_errors_batch";
    if (const std::string why = bit_errors_refusal(a_format, b_format); !why.empty())
        throw std::runtime_error(why);
    if (n && (!a_rows || !b_rows))
        throw std::runtime_error(std::string(who) + ": null operand");
    if (n == 0 || !bit_errors)
        return;
    bind_device();
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nc = static_cast<uint64_t>(plan_.nc);
    if (!gf2_tx_mask_)
    {
        std::vector<uint64_t> tx((nc + 63) / 64, 0);
        for (int c : code_->bit_pos)
            tx[static_cast<size_t>(c) / 64] |= 1ull << (c % 64);
        gf2_tx_mask_ = static_cast<const uint64_t *>(upload_table(tx.data(), tx.size() * 8, "transmitted positions"));
    }
    const uint64_t sub = gf2_sub_batch();
    const size_t a_row = bits_row_bytes(a_format, nc), b_row = bits_row_bytes(b_format, nc);
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        OutStage st;
        Gf2BitErrorArgs g{};
        g.nc = static_cast<uint32_t>(nc);
        g.tx_mask = gf2_tx_mask_;
        g.a = stage_input(static_cast<const char *>(a_rows) + a_row * done, a_row * m, stage_in_, stream);
        g.b = stage_input(static_cast<const char *>(b_rows) + b_row * done, b_row * m, stage_in_b_, stream);
        g.bit_errors = st.route(bit_errors + done, stage_gf2_[0], 4 * m);
        g.n = m;
        check(launch_gf2_bit_errors(g, a_format, b_format, s), "bit_errors_batch");
        st.flush(s, &pin_out_);
    }
}

// ---------------------------------------------------------------------------------------------
// The channel between the encoder and the decoder (kernels_channel.hip)
std::string Engine::channel_refusal(const ChannelSpec *spec, uint64_t n, int codeword_format, const void *llr, const double *received) const
{
    const std::string who = "ldpc_hip_channel_batch: ";
    if (!spec)
        return who + "null channel description";
    const ChannelSpec &c = *spec;
    if (c.channel != kAwgn && c.channel != kBsc)
        return who + "unknown channel " + std::to_string(c.channel) + " (1 = LDPC_HIP_AWGN, 2 = LDPC_HIP_BSC)";
    if (std::string why = bits_format_refusal("ldpc_hip_channel_batch", "codeword", codeword_format); !why.empty())
        return why;
    if (llr_type_bytes(c.llr_type) == 0)
        return who + "unknown LLR type " + std::to_string(c.llr_type) + " (0 = binary64, 1 = binary32, 2 = binary16, 3 = int8)";
    if (c.bits_per_symbol < 1 || c.bits_per_symbol > kChannelMaxBitsPerSymbol)
        return who + "bits_per_symbol " + std::to_string(c.bits_per_symbol) + " outside 1..4";
    if (c.channel == kBsc && c.bits_per_symbol != 1)
        return who + "the BSC carries one bit per symbol, not " + std::to_string(c.bits_per_symbol);
    if (c.channel == kAwgn && !std::isfinite(c.x))
        return who + "the AWGN point x (Es / sigma^2 in dB) is not finite";
    if (c.channel == kBsc && !(c.x > 0.0 && c.x < 1.0))
        return who + "the BSC crossover probability x is outside (0, 1)";
    if (c.llr_type == kLlrI8)
    {
        if (c.q_bits < 2 || c.q_bits > 8)
            return who + "q_bits " + std::to_string(c.q_bits) + " outside 2..8 for int8 LLRs";
        if (!(c.step >= 0x1p-20 && c.step <= 0x1p20))
            return who + "step outside [2^-20, 2^20] for int8 LLRs";
    }
    if (n && !llr && !received)
        return who + "neither llr nor received is wanted";
    return "";
}

void Engine::channel_batch(const ChannelSpec *spec, uint64_t n, const void *codeword, int codeword_format, void *llr, double *received,
                           void *stream)
{
    if (const std::string why = channel_refusal(spec, n, codeword_format, llr, received); !why.empty())
        throw std::runtime_error(why);
    if (n == 0)
        return;
    const ChannelSpec &c = *spec;
    upload_plan();
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), nct = static_cast<uint64_t>(plan_.nct);
    const int m = c.bits_per_symbol;
    if (!chan_levels_)
    {
        // the columns the channel does not write, in column order: punctured and unconnected ones get +0.0, shortened ones
        // the channel's value (plan.cpp, rank_kind: the stream's rule)
        std::vector<uint32_t> other;
        for (uint32_t col = 0; col < nc; ++col)
            if (const uint8_t kind = plan_.rank_kind[plan_.col_rank[col]]; kind != 0)
                other.push_back(col | (kind == 2 ? kChannelShortened : 0u));
        chan_n_other_ = static_cast<uint32_t>(other.size());
        chan_other_ = static_cast<const uint32_t *>(upload_table(other.data(), other.size() * 4, "columns outside the channel"));
        // 2^m-ASK of unit mean energy, m = 2..4, 16 entries each: level[j] = (M - 1 - 2 j) c, c = 1 / sqrt((M^2 - 1) / 3)
        std::vector<double> level(16 * (kChannelMaxBitsPerSymbol + 1), 0.0);
        for (int mm = 2; mm <= kChannelMaxBitsPerSymbol; ++mm)
        {
            const int M = 1 << mm;
            const double cc = 1.0 / std::sqrt(static_cast<double>(M * M - 1) / 3.0);
            for (int j = 0; j < M; ++j)
                level[16 * mm + j] = static_cast<double>(M - 1 - 2 * j) * cc;
        }
        chan_levels_ = static_cast<const double *>(upload_table(level.data(), level.size() * 8, "constellations")); // last: the mark
    }
    ChannelArgs a{};
    a.nc = static_cast<uint32_t>(nc), a.nct = static_cast<uint32_t>(nct);
    a.symbols = static_cast<uint32_t>((nct + m - 1) / m);
    a.blocks = (a.symbols + 3) / 4;
    a.n_other = chan_n_other_, a.work = a.blocks + a.n_other;
    a.bit_pos = dev_.bit_pos, a.other = chan_other_, a.level = m > 1 ? chan_levels_ + 16 * m : nullptr;
    a.codeword_format = codeword_format, a.channel = c.channel;
    a.key[0] = static_cast<uint32_t>(c.seed), a.key[1] = static_cast<uint32_t>(c.seed >> 32);
    if (c.channel == kAwgn) // the host expressions of stream_begin
    {
        a.sigma2 = std::pow(10, -c.x / 10);
        a.sigma = std::sqrt(a.sigma2);
        a.shorten = 99999.9;
    }
    else
    {
        a.eps = c.x;
        a.delta = std::log((1 - c.x) / c.x);
        a.shorten = a.delta;
    }
    a.inv = 1.0, a.qmax = 1;
    if (c.llr_type == kLlrI8)
        a.inv = 1.0 / c.step, a.qmax = (1 << (c.q_bits - 1)) - 1;
    if (a.work == 0) // (a code without columns)
        return;
    const size_t elem = llr_type_bytes(c.llr_type), in_row = bits_row_bytes(codeword_format, nc);
    // frames per launch: the staging buffers stay modest and a launch's lanes below 2^31
    const uint64_t sub = std::clamp<uint64_t>(std::min<uint64_t>((128ull << 20) / nc, ((1ull << 31) - 1) / a.work), 1, 1u << 20);
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t k = std::min(sub, n - done);
        OutStage st;
        a.codeword = codeword ? stage_input(static_cast<const char *>(codeword) + in_row * done, in_row * k, stage_in_, stream) : nullptr;
        a.llr = st.route(llr ? static_cast<char *>(llr) + elem * done * nc : nullptr, stage_chan_[0], elem * k * nc);
        a.received = st.route(received ? received + done * a.symbols : nullptr, stage_chan_[1], 8 * k * a.symbols);
        a.frame0 = c.first_frame + done;
        a.n = k;
        check(launch_channel(a, m, c.llr_type, s), "channel_batch");
        st.flush(s, &pin_out_);
    }
}

// ---------------------------------------------------------------------------------------------
// The erasure channel and the genie-free erasure decoder (kernels_erasure.hip)
std::string Engine::erasure_channel_refusal(double eps, uint64_t n, int codeword_format, const void *word_bits, const void *erased_bits) const
{
    const std::string who = "ldpc_hip_erasure_channel_batch: ";
    if (std::string why = bits_format_refusal("ldpc_hip_erasure_channel_batch", "codeword", codeword_format); !why.empty())
        return why;
    if (!(eps > 0.0 && eps < 1.0))
        return who + "the erasure probability eps is outside (0, 1)";
    if (n && !word_bits && !erased_bits)
        return who + "neither word_bits nor erased_bits is wanted";
    return "";
}

void Engine::erasure_channel_batch(double eps, uint64_t seed, uint64_t first_frame, uint64_t n, const void *codeword, int codeword_format,
                                   uint32_t *word_bits, uint32_t *erased_bits, void *stream)
{
    if (const std::string why = erasure_channel_refusal(eps, n, codeword_format, word_bits, erased_bits); !why.empty())
        throw std::runtime_error(why);
    if (n == 0)
        return;
    bind_device();
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), words = (nc + 31) / 32;
    if (!era_col_tx_)
    {
        // what each column is, by output word: transmitted (its index i < nct), punctured (erased), anything else (known) —
        // plan.cpp, rank_kind: a column in both lists counts as shortened, the surplus entries of bit_pos as never written
        std::vector<uint32_t> tx(32 * words, kErasureColPad);
        for (uint64_t c = 0; c < nc; ++c)
            tx[(c % 32) * words + c / 32] = plan_.rank_kind[plan_.col_rank[c]] == 1 ? kErasureColErased : kErasureColKnown;
        for (int i = 0; i < plan_.nct; ++i)
        {
            const uint64_t c = static_cast<uint64_t>(code_->bit_pos[i]);
            tx[(c % 32) * words + c / 32] = static_cast<uint32_t>(i);
        }
        era_col_tx_ = static_cast<const uint32_t *>(upload_table(tx.data(), tx.size() * 4, "columns of the erasure channel"));
    }
    ErasureChannelArgs a{};
    a.nc = static_cast<uint32_t>(nc), a.words = static_cast<uint32_t>(words);
    a.col_tx = era_col_tx_;
    a.codeword_format = codeword_format;
    a.key[0] = static_cast<uint32_t>(seed), a.key[1] = static_cast<uint32_t>(seed >> 32);
    a.eps = eps;
    const size_t in_row = bits_row_bytes(codeword_format, nc);
    // frames per launch: the staging buffers stay modest and a launch's lanes below 2^31
    const uint64_t sub = std::clamp<uint64_t>(std::min<uint64_t>((128ull << 20) / nc, ((1ull << 31) - 1) / words), 1, 1u << 20);
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t k = std::min(sub, n - done);
        OutStage st;
        a.codeword = codeword ? stage_input(static_cast<const char *>(codeword) + in_row * done, in_row * k, stage_in_, stream) : nullptr;
        a.word_bits = st.route(word_bits ? word_bits + done * words : nullptr, stage_era_[0], 4 * k * words);
        a.erased_bits = st.route(erased_bits ? erased_bits + done * words : nullptr, stage_era_[1], 4 * k * words);
        a.frame0 = first_frame + done;
        a.n = k;
        check(launch_erasure_channel(a, s), "erasure_channel_batch");
        st.flush(s, &pin_out_);
    }
}

// The graph cut into chunks of 64 lanes (kernels.hpp, ErasureDecodeArgs).  Host only.
const Engine::ErasureTables &Engine::erasure_tables()
{
    if (erasure_tables_)
        return *erasure_tables_;
    ErasureTables t;
    const SparseGF2 &H = code_->H;
    const uint32_t nc = static_cast<uint32_t>(plan_.nc), mc = static_cast<uint32_t>(plan_.mc);
    const auto cdeg = [&](uint32_t r) { return static_cast<uint32_t>(H.rptr[r + 1] - H.rptr[r]); };
    const auto vdeg = [&](uint32_t c) { return static_cast<uint32_t>(H.cptr[c + 1] - H.cptr[c]); };
    std::vector<uint32_t> thin, wide;
    for (uint32_t c = 0; c < nc; ++c)
        (vdeg(c) >= static_cast<uint32_t>(kErasureWideDegree) ? wide : thin).push_back(c);
    t.cn_chunks = (mc + 63) / 64;
    t.vn_chunks = static_cast<uint32_t>((wide.size() + 15) / 16 + (thin.size() + 63) / 64);
    const size_t bytes = ldpc_amd::erasure_lds_bytes(nc, mc, static_cast<size_t>(t.cn_chunks) + t.vn_chunks);
    if (nc <= 524288u && bytes <= kCuLdsBytes) // (8 (nc + 1) and 8 (mc + 1) within 160 KB: every index fits 16 bits)
    {
        t.lds_bytes = static_cast<int64_t>(bytes);
        // check nodes by degree, so that a chunk's lanes make the same trips; the slot a check node gets names it to the columns
        std::vector<uint32_t> order(mc), slot(mc);
        for (uint32_t r = 0; r < mc; ++r)
            order[r] = r;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cdeg(x) < cdeg(y); });
        for (uint32_t q = 0; q < mc; ++q)
            slot[order[q]] = q;
        for (uint32_t k = 0; k < t.cn_chunks; ++k)
        {
            const uint32_t first = 64 * k, count = std::min(64u, mc - first);
            uint32_t trips = 0;
            for (uint32_t l = 0; l < count; ++l)
                trips = std::max(trips, cdeg(order[first + l]));
            const size_t off = t.cn_entries.size();
            t.desc.push_back(static_cast<uint32_t>(off)), t.desc.push_back(trips);
            t.cn_entries.resize(off + 64 * static_cast<size_t>(trips), static_cast<uint16_t>(nc));
            for (uint32_t l = 0; l < count; ++l)
                for (uint32_t j = 0, r = order[first + l]; j < cdeg(r); ++j)
                    t.cn_entries[off + 64 * j + l] = static_cast<uint16_t>(H.rcol[H.rptr[r] + j]);
        }
        // columns: the wide ones first (four lanes each, 16 to a chunk), then the thin ones, each kind by degree
        const auto by_degree = [&](uint32_t x, uint32_t y) { return vdeg(x) > vdeg(y); };
        std::stable_sort(wide.begin(), wide.end(), by_degree);
        std::stable_sort(thin.begin(), thin.end(), by_degree);
        const auto add = [&](const std::vector<uint32_t> &cols, uint32_t per_chunk, uint32_t lanes_per_col) {
            for (size_t first = 0; first < cols.size(); first += per_chunk)
            {
                const uint32_t count = static_cast<uint32_t>(std::min<size_t>(per_chunk, cols.size() - first));
                uint32_t trips = 0;
                for (uint32_t i = 0; i < count; ++i)
                    trips = std::max(trips, (vdeg(cols[first + i]) + lanes_per_col - 1) / lanes_per_col);
                const size_t off = t.vn_entries.size(), at = t.vn_col.size();
                t.desc.push_back(static_cast<uint32_t>(off)), t.desc.push_back(trips | (lanes_per_col > 1 ? kErasureWideChunk : 0u));
                t.vn_entries.resize(off + 64 * static_cast<size_t>(trips), static_cast<uint16_t>(mc));
                t.vn_col.resize(at + 64, static_cast<uint16_t>(nc));
                for (uint32_t i = 0; i < count; ++i)
                {
                    const uint32_t c = cols[first + i];
                    for (uint32_t sub = 0; sub < lanes_per_col; ++sub)
                        t.vn_col[at + lanes_per_col * i + sub] = static_cast<uint16_t>(c);
                    for (uint32_t p = 0; p < vdeg(c); ++p)
                        t.vn_entries[off + 64 * (p / lanes_per_col) + lanes_per_col * i + p % lanes_per_col] =
                            static_cast<uint16_t>(slot[H.crow[H.cptr[c] + p]]);
                }
            }
        };
        add(wide, 16, 4);
        add(thin, 64, 1);
    }
    erasure_tables_ = std::move(t);
    return *erasure_tables_;
}

int64_t Engine::erasure_lds_bytes() { return erasure_tables().lds_bytes; }

std::string Engine::erasure_decode_refusal(int flags, int format)
{
    const std::string who = "ldpc_hip_erasure_decode_batch: ";
    if (std::string why = bits_format_refusal("ldpc_hip_erasure_decode_batch", "word and erased", format); !why.empty())
        return why;
    if (flags & ~(kErasureEarlyTerm | kErasureStopStalled))
        return who + "unknown flags " + std::to_string(flags) + " (1 = LDPC_HIP_ERASURE_EARLY_TERM, 2 = LDPC_HIP_ERASURE_STOP_STALLED)";
    if (plan_.nc > 524288)
        return who + "more than 524 288 columns";
    if (erasure_lds_bytes() < 0)
        return who + "a group of 32 frames does not fit the 160 KB of LDS of a CU (ldpc_hip_erasure_lds_bytes; there is no other kernel)";
    return "";
}

void Engine::erasure_decode_batch(uint32_t iterations, int flags, uint64_t n, const void *word, const void *erased, int format,
                                  uint32_t *word_out, uint32_t *erased_out, uint32_t *iters, uint32_t *unresolved, void *stream)
{
    if (const std::string why = erasure_decode_refusal(flags, format); !why.empty())
        throw std::runtime_error(why);
    if (n && (!word || !erased))
        throw std::runtime_error("ldpc_hip_erasure_decode_batch: null word or erased");
    if (n == 0 || (!word_out && !erased_out && !iters && !unresolved))
        return;
    bind_device();
    hipStream_t s = static_cast<hipStream_t>(stream);
    const ErasureTables &t = erasure_tables();
    if (!era_desc_)
    {
        era_cn_entries_ = static_cast<const uint16_t *>(upload_table(t.cn_entries.data(), t.cn_entries.size() * 2, "erasure graph"));
        era_vn_entries_ = static_cast<const uint16_t *>(upload_table(t.vn_entries.data(), t.vn_entries.size() * 2, "erasure graph"));
        era_vn_col_ = static_cast<const uint16_t *>(upload_table(t.vn_col.data(), t.vn_col.size() * 2, "erasure graph"));
        era_desc_ = static_cast<const uint32_t *>(upload_table(t.desc.data(), t.desc.size() * 4, "erasure graph")); // last: the mark
    }
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), words = (nc + 31) / 32;
    ErasureDecodeArgs a{};
    a.nc = static_cast<uint32_t>(nc), a.mc = static_cast<uint32_t>(plan_.mc), a.words = static_cast<uint32_t>(words);
    a.cn_chunks = t.cn_chunks, a.vn_chunks = t.vn_chunks;
    a.iterations = iterations, a.flags = flags;
    a.lds_bytes = static_cast<uint32_t>(t.lds_bytes);
    a.desc = era_desc_, a.cn_entries = era_cn_entries_, a.vn_entries = era_vn_entries_, a.vn_col = era_vn_col_;
    const uint64_t sub = gf2_sub_batch();
    const size_t in_row = bits_row_bytes(format, nc);
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        const void *src[2] = {stage_input(static_cast<const char *>(word) + in_row * done, in_row * m, stage_in_, stream),
                              stage_input(static_cast<const char *>(erased) + in_row * done, in_row * m, stage_in_b_, stream)};
        if (format == kBitsU8) // bytes: packed by one small launch each in front
            for (int i = 0; i < 2; ++i)
            {
                uint32_t *packed = static_cast<uint32_t *>(era_packed_[i].reserve(4 * m * words));
                check(launch_pack_hard(static_cast<const uint8_t *>(src[i]), m, static_cast<int>(nc), packed, s), "erasure_decode_batch (pack)");
                src[i] = packed;
            }
        OutStage st;
        a.word = static_cast<const uint32_t *>(src[0]), a.erased = static_cast<const uint32_t *>(src[1]);
        a.word_out = st.route(word_out ? word_out + done * words : nullptr, stage_era_[0], 4 * m * words);
        a.erased_out = st.route(erased_out ? erased_out + done * words : nullptr, stage_era_[1], 4 * m * words);
        a.iters = st.route(iters ? iters + done : nullptr, stage_era_[2], 4 * m);
        a.unresolved = st.route(unresolved ? unresolved + done : nullptr, stage_era_[3], 4 * m);
        a.n = m;
        check(launch_erasure_decode(a, s), "erasure_decode_batch");
        st.flush(s, &pin_out_);
    }
}

// ---------------------------------------------------------------------------------------------
// Maximum-likelihood erasure decoding (kernels_erasure_solve.hip)
int64_t Engine::erasure_solve_lds_bytes(uint32_t max_unknowns) const
{
    if (max_unknowns == 0)
        return -1;
    const size_t nc = static_cast<size_t>(plan_.nc), mc = static_cast<size_t>(plan_.mc), cap = std::min<size_t>(max_unknowns, nc);
    const size_t bytes = ldpc_amd::erasure_solve_lds_bytes(nc, mc, cap, erasure_solve_rows(mc, cap, static_cast<size_t>(plan_.max_vn_degree)));
    return bytes <= kCuLdsBytes ? static_cast<int64_t>(bytes) : -1;
}

std::string Engine::erasure_solve_refusal(uint32_t max_unknowns, int format) const
{
    const std::string who = "ldpc_hip_erasure_solve_batch: ";
    if (std::string why = bits_format_refusal("ldpc_hip_erasure_solve_batch", "word and erased", format); !why.empty())
        return why;
    if (max_unknowns == 0)
        return who + "max_unknowns is 0";
    if (erasure_solve_lds_bytes(max_unknowns) < 0)
        return who + "a frame of " + std::to_string(std::min<uint64_t>(max_unknowns, static_cast<uint64_t>(plan_.nc))) +
               " unknowns does not fit the 160 KB of LDS of a CU (ldpc_hip_erasure_solve_lds_bytes; there is no other kernel)";
    return "";
}

void Engine::erasure_solve_batch(uint32_t max_unknowns, uint64_t n, const void *word, const void *erased, int format, uint32_t *word_out,
                                 uint32_t *erased_out, uint32_t *unresolved, uint32_t *rank, uint32_t *status, void *stream)
{
    if (const std::string why = erasure_solve_refusal(max_unknowns, format); !why.empty())
        throw std::runtime_error(why);
    if (n && (!word || !erased))
        throw std::runtime_error("ldpc_hip_erasure_solve_batch: null word or erased");
    if (n == 0 || (!word_out && !erased_out && !unresolved && !rank && !status))
        return;
    bind_device();
    hipStream_t s = static_cast<hipStream_t>(stream);
    upload_rows_of_h();
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), mc = static_cast<uint64_t>(plan_.mc), words = (nc + 31) / 32;
    ErasureSolveArgs a{};
    a.nc = static_cast<uint32_t>(nc), a.mc = static_cast<uint32_t>(mc), a.words = static_cast<uint32_t>(words);
    a.cap = static_cast<uint32_t>(std::min<uint64_t>(max_unknowns, nc));
    a.rows = static_cast<uint32_t>(erasure_solve_rows(mc, a.cap, static_cast<size_t>(plan_.max_vn_degree)));
    a.threads = std::clamp<uint32_t>((a.rows + 63u) / 64u * 64u, 64u, kErasureSolveMaxThreads); // a thread per row where they reach
    a.lds_bytes = static_cast<uint32_t>(erasure_solve_lds_bytes(max_unknowns));
    a.row_ptr = gf2_row_ptr_, a.row_col = gf2_row_col_;
    const uint64_t sub = gf2_sub_batch();
    const size_t in_row = bits_row_bytes(format, nc);
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        const void *src[2] = {stage_input(static_cast<const char *>(word) + in_row * done, in_row * m, stage_in_, stream),
                              stage_input(static_cast<const char *>(erased) + in_row * done, in_row * m, stage_in_b_, stream)};
        if (format == kBitsU8) // bytes: packed by one small launch each in front
            for (int i = 0; i < 2; ++i)
            {
                uint32_t *packed = static_cast<uint32_t *>(era_packed_[i].reserve(4 * m * words));
                check(launch_pack_hard(static_cast<const uint8_t *>(src[i]), m, static_cast<int>(nc), packed, s), "erasure_solve_batch (pack)");
                src[i] = packed;
            }
        OutStage st;
        a.word = static_cast<const uint32_t *>(src[0]), a.erased = static_cast<const uint32_t *>(src[1]);
        a.word_out = st.route(word_out ? word_out + done * words : nullptr, stage_era_[0], 4 * m * words);
        a.erased_out = st.route(erased_out ? erased_out + done * words : nullptr, stage_era_[1], 4 * m * words);
        a.unresolved = st.route(unresolved ? unresolved + done : nullptr, stage_era_[2], 4 * m);
        a.rank = st.route(rank ? rank + done : nullptr, stage_era_[3], 4 * m);
        a.status = st.route(status ? status + done : nullptr, stage_era_[4], 4 * m);
        a.n = m;
        check(launch_erasure_solve(a, s), "erasure_solve_batch");
        st.flush(s, &pin_out_);
    }
}

// ---------------------------------------------------------------------------------------------
// Ordered-statistics decoding (kernels_osd.hip)
int64_t Engine::osd_lds_bytes() const
{
    const size_t nc = static_cast<size_t>(plan_.nc), mc = static_cast<size_t>(plan_.mc);
    if (nc > 0xFFFFu || mc > static_cast<size_t>(kOsdRowsPerThread) * kOsdMaxThreads) // (the order is 16 bits a column)
        return -1;
    const size_t bytes = ldpc_amd::osd_lds_bytes(nc, mc);
    return bytes <= kCuLdsBytes ? static_cast<int64_t>(bytes) : -1;
}

std::string Engine::osd_refusal(int llr_type) const
{
    const std::string who = "ldpc_hip_osd_batch: ";
    if (llr_type_bytes(llr_type) == 0)
        return who + "unknown LLR type " + std::to_string(llr_type) + " (0 = binary64, 1 = binary32, 2 = binary16, 3 = int8)";
    if (osd_lds_bytes() < 0)
        return who + "the check matrix of " + std::to_string(plan_.mc) + " x " + std::to_string(plan_.nc) +
               " bits does not fit the 160 KB of LDS of a CU (ldpc_hip_osd_lds_bytes; there is no other kernel)";
    return "";
}

void Engine::osd_batch(uint32_t candidates, uint64_t n, const void *llr, int llr_type, uint32_t *word_out, uint32_t *flips, uint64_t *metric,
                       uint32_t *flipped_column, uint32_t *status, void *stream)
{
    if (const std::string why = osd_refusal(llr_type); !why.empty())
        throw std::runtime_error(why);
    if (n && !llr)
        throw std::runtime_error("ldpc_hip_osd_batch: null llr");
    if (n == 0 || (!word_out && !flips && !metric && !flipped_column && !status))
        return;
    bind_device();
    hipStream_t s = static_cast<hipStream_t>(stream);
    upload_rows_of_h();
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), mc = static_cast<uint64_t>(plan_.mc), words = (nc + 31) / 32;
    OsdArgs a{};
    a.nc = static_cast<uint32_t>(nc), a.mc = static_cast<uint32_t>(mc), a.words = static_cast<uint32_t>(words);
    a.candidates = candidates, a.llr_type = llr_type;
    a.threads = std::clamp<uint32_t>((a.mc + 63u) / 64u * 64u, 64u, kOsdMaxThreads); // a thread per row where they reach
    a.lds_bytes = static_cast<uint32_t>(osd_lds_bytes());
    a.row_ptr = gf2_row_ptr_, a.row_col = gf2_row_col_;
    const uint64_t sub = std::max<uint64_t>(gf2_sub_batch() / llr_type_bytes(llr_type), 1); // (elements of up to 8 bytes, not bits)
    const size_t in_row = llr_type_bytes(llr_type) * nc;
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        a.llr = stage_input(static_cast<const char *>(llr) + in_row * done, in_row * m, llr_type == kLlrF64 ? stage_in_ : stage_typed_, stream);
        OutStage st;
        a.word_out = st.route(word_out ? word_out + done * words : nullptr, stage_osd_[0], 4 * m * words);
        a.flips = st.route(flips ? flips + done : nullptr, stage_osd_[1], 4 * m);
        a.metric = st.route(metric ? metric + done : nullptr, stage_osd_[2], 8 * m);
        a.flipped_column = st.route(flipped_column ? flipped_column + done : nullptr, stage_osd_[3], 4 * m);
        a.status = st.route(status ? status + done : nullptr, stage_osd_[4], 4 * m);
        a.n = m;
        check(launch_osd(a, s), "osd_batch");
        st.flush(s, &pin_out_);
    }
}

// ---------------------------------------------------------------------------------------------
// Ordered-statistics decoding toward a given syndrome, singles and a bounded pair sweep (kernels_osd_syndrome.hip)
int64_t Engine::osd_syndrome_lds_bytes() const
{
    const size_t nc = static_cast<size_t>(plan_.nc), mc = static_cast<size_t>(plan_.mc);
    if (nc > 0xFFFFu || mc > static_cast<size_t>(kOsdRowsPerThread) * kOsdMaxThreads) // (the order is 16 bits a column)
        return -1;
    const size_t bytes = ldpc_amd::osd_syndrome_lds_bytes(nc, mc);
    return bytes <= kCuLdsBytes ? static_cast<int64_t>(bytes) : -1;
}

std::string Engine::osd_syndrome_refusal(uint32_t pair_depth, int llr_type, int syndrome_format) const
{
    const std::string who = "ldpc_hip_osd_syndrome_batch: ";
    if (llr_type_bytes(llr_type) == 0)
        return who + "unknown LLR type " + std::to_string(llr_type) + " (0 = binary64, 1 = binary32, 2 = binary16, 3 = int8)";
    if (std::string why = bits_format_refusal("ldpc_hip_osd_syndrome_batch", "syndrome", syndrome_format); !why.empty())
        return why;
    if (pair_depth > kOsdMaxPairDepth)
        return who + "pair_depth " + std::to_string(pair_depth) + " is beyond " + std::to_string(kOsdMaxPairDepth) +
               " (32 640 pairs a frame)";
    if (osd_syndrome_lds_bytes() < 0)
        return who + "the check matrix of " + std::to_string(plan_.mc) + " x " + std::to_string(plan_.nc) +
               " bits does not fit the 160 KB of LDS of a CU (ldpc_hip_osd_syndrome_lds_bytes; there is no other kernel)";
    return "";
}

void Engine::osd_syndrome_batch(uint32_t candidates, uint32_t pair_depth, uint64_t n, const void *llr, int llr_type, const void *syndrome,
                                int syndrome_format, uint32_t *word_out, uint32_t *flips, uint64_t *metric, uint32_t *flipped_columns,
                                uint32_t *status, void *stream)
{
    if (const std::string why = osd_syndrome_refusal(pair_depth, llr_type, syndrome_format); !why.empty())
        throw std::runtime_error(why);
    if (n && !llr)
        throw std::runtime_error("ldpc_hip_osd_syndrome_batch: null llr");
    if (n == 0 || (!word_out && !flips && !metric && !flipped_columns && !status))
        return;
    bind_device();
    hipStream_t s = static_cast<hipStream_t>(stream);
    upload_rows_of_h();
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), mc = static_cast<uint64_t>(plan_.mc), words = (nc + 31) / 32;
    OsdSyndromeArgs a{};
    a.nc = static_cast<uint32_t>(nc), a.mc = static_cast<uint32_t>(mc), a.words = static_cast<uint32_t>(words);
    a.syn_words = static_cast<uint32_t>((mc + 31) / 32);
    a.candidates = candidates, a.pair_depth = pair_depth, a.llr_type = llr_type, a.syndrome_format = syndrome_format;
    a.threads = std::clamp<uint32_t>((a.mc + 63u) / 64u * 64u, 64u, kOsdMaxThreads); // a thread per row where they reach
    a.lds_bytes = static_cast<uint32_t>(osd_syndrome_lds_bytes());
    a.row_ptr = gf2_row_ptr_, a.row_col = gf2_row_col_;
    const uint64_t sub = std::max<uint64_t>(gf2_sub_batch() / llr_type_bytes(llr_type), 1); // (elements of up to 8 bytes, not bits)
    const size_t in_row = llr_type_bytes(llr_type) * nc, syn_row = bits_row_bytes(syndrome_format, mc);
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        a.llr = stage_input(static_cast<const char *>(llr) + in_row * done, in_row * m, llr_type == kLlrF64 ? stage_in_ : stage_typed_, stream);
        a.syndrome = syndrome ? stage_input(static_cast<const char *>(syndrome) + syn_row * done, syn_row * m, stage_in_b_, stream) : nullptr;
        OutStage st;
        a.word_out = st.route(word_out ? word_out + done * words : nullptr, stage_osd_[0], 4 * m * words);
        a.flips = st.route(flips ? flips + done : nullptr, stage_osd_[1], 4 * m);
        a.metric = st.route(metric ? metric + done : nullptr, stage_osd_[2], 8 * m);
        a.flipped_columns = st.route(flipped_columns ? flipped_columns + 2 * done : nullptr, stage_osd_[3], 8 * m);
        a.status = st.route(status ? status + done : nullptr, stage_osd_[4], 4 * m);
        a.n = m;
        check(launch_osd_syndrome(a, s), "osd_syndrome_batch");
        st.flush(s, &pin_out_);
    }
}

// ---------------------------------------------------------------------------------------------
// Quantized min-sum decoding toward a given syndrome (kernels_syndrome_decode.hip)
int64_t Engine::syndrome_decode_lds_bytes()
{
    const QmsPlan &q = qms_plan();
    if (!q.ok || plan_.nc > 0xFFFF || plan_.mc <= 0)
        return -1;
    const size_t bytes = ldpc_amd::syndrome_decode_lds_bytes(q.slots, static_cast<size_t>(plan_.nc), static_cast<size_t>(plan_.mc));
    return bytes <= kCuLdsBytes ? static_cast<int64_t>(bytes) : -1;
}

std::string Engine::syndrome_decode_refusal(const SyndromeDecodeSpec *spec, int llr_type, int syndrome_format)
{
    const std::string who = "ldpc_hip_syndrome_decode_batch: ";
    if (!spec)
        return who + "null parameters";
    if (spec->q_bits < 2 || spec->q_bits > 8)
        return who + "q_bits " + std::to_string(spec->q_bits) + " is outside 2..8";
    if (!(spec->step > 0.0) || spec->step < 0x1p-20 || spec->step > 0x1p20) // (a NaN fails the first)
        return who + "the step must lie in [2^-20, 2^20]";
    if (!(spec->scale > 0.0) || spec->scale > 1.0)
        return who + "the scale must lie in (0, 1]";
    if (!(spec->offset >= 0.0) || spec->offset > 1e6)
        return who + "the offset must lie in [0, 1e6]";
    if (spec->early_term != 0 && spec->early_term != 1)
        return who + "early_term " + std::to_string(spec->early_term) + " is neither 0 nor 1";
    if (spec->flags & ~kSyndromeSharedLlr)
        return who + "unknown flag bits " + std::to_string(spec->flags & ~kSyndromeSharedLlr);
    if (llr_type_bytes(llr_type) == 0)
        return who + "unknown LLR type " + std::to_string(llr_type) + " (0 = binary64, 1 = binary32, 2 = binary16, 3 = int8)";
    if (std::string why = bits_format_refusal("ldpc_hip_syndrome_decode_batch", "syndrome", syndrome_format); !why.empty())
        return why;
    if (syndrome_decode_lds_bytes() < 0)
        return who + "the code of " + std::to_string(plan_.mc) + " x " + std::to_string(plan_.nc) +
               " is not taken: more than 65 535 columns, a check node with fewer than two entries, or a frame beyond the 160 KB of LDS "
               "of a CU (ldpc_hip_syndrome_decode_lds_bytes; there is no other kernel)";
    return "";
}

void Engine::syndrome_decode_batch(const SyndromeDecodeSpec *spec, uint64_t n, const void *llr, int llr_type, const void *syndrome,
                                   int syndrome_format, uint32_t *hard_bits, uint32_t *iters, uint32_t *weight, double *llr_out, void *stream)
{
    if (const std::string why = syndrome_decode_refusal(spec, llr_type, syndrome_format); !why.empty())
        throw std::runtime_error(why);
    if (n && !llr)
        throw std::runtime_error("ldpc_hip_syndrome_decode_batch: null llr");
    if (n == 0 || (!hard_bits && !iters && !weight && !llr_out))
        return;
    upload_plan();
    upload_qms_plan();
    if (!sd_cn_row_)
        sd_cn_row_ = static_cast<const uint32_t *>(upload_table(plan_.cn_rank_row.data(), plan_.cn_rank_row.size() * 4, "check node order"));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), mc = static_cast<uint64_t>(plan_.mc), words = (nc + 31) / 32;
    const bool shared = (spec->flags & kSyndromeSharedLlr) != 0;
    SyndromeDecodeArgs a{};
    a.nc = static_cast<uint32_t>(nc), a.mc = static_cast<uint32_t>(mc), a.words = static_cast<uint32_t>(words);
    a.syn_words = static_cast<uint32_t>((mc + 31) / 32);
    a.iterations = spec->iterations, a.early_term = spec->early_term;
    a.llr_type = llr_type, a.syndrome_format = syndrome_format, a.shared_llr = shared ? 1 : 0;
    {
        const QmsArgs q = quantizer_args<QmsArgs>(spec->step, spec->q_bits, spec->scale, spec->offset); // (the same host routine)
        a.qmax = q.qmax, a.step = q.step, a.inv = q.inv;
        std::memcpy(a.lut, q.lut, sizeof a.lut);
    }
    a.lds_bytes = static_cast<uint32_t>(syndrome_decode_lds_bytes());
    a.col_rank = dev_.col_rank, a.cn_row = sd_cn_row_;
    const size_t elem = llr_type_bytes(llr_type), in_row = elem * nc, syn_row = bits_row_bytes(syndrome_format, mc);
    DeviceBuffer &llr_stage = llr_type == kLlrF64 ? stage_in_ : stage_typed_;
    if (shared) // one row for every frame: staged once
        a.llr = stage_input(llr, in_row, llr_stage, stream);
    const uint64_t sub = std::max<uint64_t>(gf2_sub_batch() / elem, 1); // (elements of up to 8 bytes, not bits)
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        if (!shared)
            a.llr = stage_input(static_cast<const char *>(llr) + in_row * done, in_row * m, llr_stage, stream);
        a.syndrome = syndrome ? stage_input(static_cast<const char *>(syndrome) + syn_row * done, syn_row * m, stage_in_b_, stream) : nullptr;
        OutStage st;
        a.hard_bits = st.route(hard_bits ? hard_bits + done * words : nullptr, stage_sd_[0], 4 * m * words);
        a.iters = st.route(iters ? iters + done : nullptr, stage_sd_[1], 4 * m);
        a.weight = st.route(weight ? weight + done : nullptr, stage_sd_[2], 4 * m);
        a.llr_out = st.route(llr_out ? llr_out + done * nc : nullptr, stage_sd_[3], 8 * m * nc);
        a.n = m;
        check(launch_syndrome_decode(a, dev_qms_, s), "syndrome_decode_batch");
        st.flush(s, &pin_out_);
    }
}

// ---------------------------------------------------------------------------------------------
// Fixed-point layered min-sum decoding toward a given syndrome (kernels_syndrome_decode_layered.hip)
int64_t Engine::syndrome_decode_layered_lds_bytes()
{
    const int64_t bytes = plan_.mc <= 0 ? -1 : layered_fixed_direct_lds_bytes(); // (the syndrome rides in the records: no byte more)
    return bytes <= static_cast<int64_t>(kCuLdsBytes) ? bytes : -1;
}

std::string Engine::syndrome_decode_layered_refusal(const SyndromeDecodeLayeredSpec *spec, int llr_type, int syndrome_format)
{
    const char *entry = "ldpc_hip_syndrome_decode_layered_batch";
    const std::string who = std::string(entry) + ": ";
    if (!spec)
        return who + "null parameters";
    if (spec->msg_bits < 2 || spec->msg_bits > 8)
        return who + "msg_bits " + std::to_string(spec->msg_bits) + " is outside 2..8";
    if (spec->app_bits < spec->msg_bits || spec->app_bits > 16)
        return who + "app_bits " + std::to_string(spec->app_bits) + " is outside msg_bits..16";
    if (!(spec->step > 0.0) || spec->step < 0x1p-20 || spec->step > 0x1p20) // (a NaN fails the first)
        return who + "the step must lie in [2^-20, 2^20]";
    if (!(spec->scale > 0.0) || spec->scale > 1.0)
        return who + "the scale must lie in (0, 1]";
    if (!(spec->offset >= 0.0) || spec->offset > 1e6)
        return who + "the offset must lie in [0, 1e6]";
    if (spec->early_term != 0 && spec->early_term != 1)
        return who + "early_term " + std::to_string(spec->early_term) + " is neither 0 nor 1";
    if (spec->flags & ~kSyndromeSharedLlr)
        return who + "unknown flag bits " + std::to_string(spec->flags & ~kSyndromeSharedLlr);
    if (llr_type_bytes(llr_type) == 0)
        return who + "unknown LLR type " + std::to_string(llr_type) + " (0 = binary64, 1 = binary32, 2 = binary16, 3 = int8)";
    if (std::string why = bits_format_refusal(entry, "syndrome", syndrome_format); !why.empty())
        return why;
    if (syndrome_decode_layered_lds_bytes() < 0)
        return who + "the code of " + std::to_string(plan_.mc) + " x " + std::to_string(plan_.nc) +
               " is not taken: the layered schedule takes codes whose check nodes all have degree 2..8, with at most 65 535 columns and no "
               "isolated variable node, and a frame within the 160 KB of LDS of a CU (ldpc_hip_syndrome_decode_layered_lds_bytes; there is "
               "no other kernel)";
    return "";
}

void Engine::syndrome_decode_layered_batch(const SyndromeDecodeLayeredSpec *spec, uint64_t n, const void *llr, int llr_type,
                                           const void *syndrome, int syndrome_format, uint32_t *hard_bits, uint32_t *iters, uint32_t *weight,
                                           double *llr_out, void *stream)
{
    if (const std::string why = syndrome_decode_layered_refusal(spec, llr_type, syndrome_format); !why.empty())
        throw std::runtime_error(why);
    if (n && !llr)
        throw std::runtime_error("ldpc_hip_syndrome_decode_layered_batch: null llr");
    if (n == 0 || (!hard_bits && !iters && !weight && !llr_out))
        return;
    upload_plan();
    upload_layer_plan();
    if (!sdl_step_row_) // lane l of step s holds the l-th of the step's check nodes in file order (plan.cpp, build_layer_plan)
    {
        const LayerPlan &L = layer_plan();
        std::vector<uint32_t> step_row(L.steps.size() * kWaveSize, 0), filled(L.steps.size(), 0);
        for (size_t row = 0; row < L.step_of_row.size(); ++row)
        {
            const size_t si = static_cast<size_t>(L.step_of_row[row]);
            step_row[si * kWaveSize + filled[si]++] = static_cast<uint32_t>(row);
        }
        sdl_step_row_ = static_cast<const uint32_t *>(upload_table(step_row.data(), step_row.size() * 4, "check nodes of the steps"));
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), mc = static_cast<uint64_t>(plan_.mc), words = (nc + 31) / 32;
    const bool shared = (spec->flags & kSyndromeSharedLlr) != 0;
    SyndromeDecodeLayeredArgs a{};
    a.nc = static_cast<uint32_t>(nc), a.mc = static_cast<uint32_t>(mc), a.words = static_cast<uint32_t>(words);
    a.syn_words = static_cast<uint32_t>((mc + 31) / 32);
    a.iterations = spec->iterations, a.early_term = spec->early_term;
    a.llr_type = llr_type, a.syndrome_format = syndrome_format, a.shared_llr = shared ? 1 : 0;
    a.q = quantizer_args<LayeredFixedArgs>(spec->step, spec->msg_bits, spec->scale, spec->offset); // (the same host routine)
    a.q.pmax = (1 << (spec->app_bits - 1)) - 1;
    a.lds_bytes = static_cast<uint32_t>(syndrome_decode_layered_lds_bytes());
    a.col_rank = dev_.col_rank, a.step_row = sdl_step_row_;
    const size_t elem = llr_type_bytes(llr_type), in_row = elem * nc, syn_row = bits_row_bytes(syndrome_format, mc);
    DeviceBuffer &llr_stage = llr_type == kLlrF64 ? stage_in_ : stage_typed_;
    if (shared) // one row for every frame: staged once
        a.llr = stage_input(llr, in_row, llr_stage, stream);
    const uint64_t sub = std::max<uint64_t>(gf2_sub_batch() / elem, 1); // (elements of up to 8 bytes, not bits)
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        if (!shared)
            a.llr = stage_input(static_cast<const char *>(llr) + in_row * done, in_row * m, llr_stage, stream);
        a.syndrome = syndrome ? stage_input(static_cast<const char *>(syndrome) + syn_row * done, syn_row * m, stage_in_b_, stream) : nullptr;
        OutStage st;
        a.hard_bits = st.route(hard_bits ? hard_bits + done * words : nullptr, stage_sd_[0], 4 * m * words);
        a.iters = st.route(iters ? iters + done : nullptr, stage_sd_[1], 4 * m);
        a.weight = st.route(weight ? weight + done : nullptr, stage_sd_[2], 4 * m);
        a.llr_out = st.route(llr_out ? llr_out + done * nc : nullptr, stage_sd_[3], 8 * m * nc);
        a.n = m;
        check(launch_syndrome_decode_layered(a, dev_layer_, s), "syndrome_decode_layered_batch");
        st.flush(s, &pin_out_);
    }
}

// ---------------------------------------------------------------------------------------------
// Gradient-descent bit flipping toward a given syndrome (kernels_bit_flip.hip)
int64_t Engine::bit_flip_lds_bytes() const
{
    if (plan_.nc <= 0 || plan_.nc > 0xFFFF || plan_.mc <= 0 || plan_.mc > 0xFFFF) // (the tables hold 16-bit indices)
        return -1;
    const size_t bytes = ldpc_amd::bit_flip_lds_bytes(static_cast<size_t>(plan_.nc), static_cast<size_t>(plan_.mc));
    return bytes <= kCuLdsBytes ? static_cast<int64_t>(bytes) : -1;
}

std::string Engine::bit_flip_refusal(const BitFlipSpec *spec, int llr_type, int syndrome_format) const
{
    const char *entry = "ldpc_hip_bit_flip_batch";
    const std::string who = std::string(entry) + ": ";
    if (!spec)
        return who + "null parameters";
    if (spec->iterations > 0xFFFFu)
        return who + "iterations " + std::to_string(spec->iterations) + " is beyond 65535";
    if (spec->q_bits < 2 || spec->q_bits > 8)
        return who + "q_bits " + std::to_string(spec->q_bits) + " is outside 2..8";
    if (!(spec->step > 0.0) || spec->step < 0x1p-20 || spec->step > 0x1p20) // (a NaN fails the first)
        return who + "the step must lie in [2^-20, 2^20]";
    if (spec->check_weight < 1 || spec->check_weight > 255)
        return who + "check_weight " + std::to_string(spec->check_weight) + " is outside 1..255";
    if (spec->margin > 0xFFFFu)
        return who + "margin " + std::to_string(spec->margin) + " is beyond 65535";
    if (spec->flags & ~kSyndromeSharedLlr)
        return who + "unknown flag bits " + std::to_string(spec->flags & ~kSyndromeSharedLlr);
    if (llr_type_bytes(llr_type) == 0)
        return who + "unknown LLR type " + std::to_string(llr_type) + " (0 = binary64, 1 = binary32, 2 = binary16, 3 = int8)";
    if (std::string why = bits_format_refusal(entry, "syndrome", syndrome_format); !why.empty())
        return why;
    if (bit_flip_lds_bytes() < 0)
        return who + "the code of " + std::to_string(plan_.mc) + " x " + std::to_string(plan_.nc) +
               " is not taken: more than 65 535 columns or check nodes, or a frame beyond the 160 KB of LDS of a CU "
               "(ldpc_hip_bit_flip_lds_bytes; there is no other kernel)";
    return "";
}

void Engine::bit_flip_batch(const BitFlipSpec *spec, uint64_t n, const void *llr, int llr_type, const void *syndrome, int syndrome_format,
                            uint32_t *hard_bits, uint32_t *iters, uint32_t *weight, void *stream)
{
    if (const std::string why = bit_flip_refusal(spec, llr_type, syndrome_format); !why.empty())
        throw std::runtime_error(why);
    if (n && !llr)
        throw std::runtime_error("ldpc_hip_bit_flip_batch: null llr");
    if (n == 0 || (!hard_bits && !iters && !weight))
        return;
    bind_device();
    if (!bf_row_ptr_) // H by rows and by columns, each in file order, repeated entries included
    {
        const SparseGF2 &H = code_->H;
        const std::vector<uint32_t> rp(H.rptr.begin(), H.rptr.end()), cp(H.cptr.begin(), H.cptr.end());
        const std::vector<uint16_t> rc(H.rcol.begin(), H.rcol.end()), cr(H.crow.begin(), H.crow.end());
        bf_row_col_ = static_cast<const uint16_t *>(upload_table(rc.data(), rc.size() * 2, "rows of H (16 bits)"));
        bf_col_row_ = static_cast<const uint16_t *>(upload_table(cr.data(), cr.size() * 2, "columns of H (16 bits)"));
        bf_col_ptr_ = static_cast<const uint32_t *>(upload_table(cp.data(), cp.size() * 4, "columns of H (16 bits)"));
        bf_row_ptr_ = static_cast<const uint32_t *>(upload_table(rp.data(), rp.size() * 4, "rows of H (16 bits)")); // last: the mark
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), mc = static_cast<uint64_t>(plan_.mc), words = (nc + 31) / 32;
    const bool shared = (spec->flags & kSyndromeSharedLlr) != 0;
    BitFlipArgs a{};
    a.nc = static_cast<uint32_t>(nc), a.mc = static_cast<uint32_t>(mc), a.words = static_cast<uint32_t>(words);
    a.syn_words = static_cast<uint32_t>((mc + 31) / 32);
    a.iterations = spec->iterations;
    a.llr_type = llr_type, a.syndrome_format = syndrome_format, a.shared_llr = shared ? 1 : 0;
    a.qmax = (1 << (spec->q_bits - 1)) - 1, a.inv = 1.0 / spec->step; // (the quantizer of quantizer_args)
    a.check_weight = static_cast<int32_t>(spec->check_weight), a.margin = static_cast<int32_t>(spec->margin);
    a.flip_threshold = spec->flip_threshold;
    a.k0 = static_cast<uint32_t>(spec->seed), a.k1 = static_cast<uint32_t>(spec->seed >> 32);
    a.draw_blocks = static_cast<uint32_t>((nc + 3) / 4);
    a.frame_bytes = static_cast<uint32_t>(bit_flip_lds_bytes());
    a.group_frames = bit_flip_group_frames(a.frame_bytes);
    a.row_ptr = bf_row_ptr_, a.row_col = bf_row_col_, a.col_ptr = bf_col_ptr_, a.col_row = bf_col_row_;
    const size_t elem = llr_type_bytes(llr_type), in_row = elem * nc, syn_row = bits_row_bytes(syndrome_format, mc);
    DeviceBuffer &llr_stage = llr_type == kLlrF64 ? stage_in_ : stage_typed_;
    if (shared) // one row for every frame: staged once
        a.llr = stage_input(llr, in_row, llr_stage, stream);
    const uint64_t sub = std::max<uint64_t>(gf2_sub_batch() / elem, 1); // (elements of up to 8 bytes, not bits)
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        if (!shared)
            a.llr = stage_input(static_cast<const char *>(llr) + in_row * done, in_row * m, llr_stage, stream);
        a.syndrome = syndrome ? stage_input(static_cast<const char *>(syndrome) + syn_row * done, syn_row * m, stage_in_b_, stream) : nullptr;
        OutStage st;
        a.hard_bits = st.route(hard_bits ? hard_bits + done * words : nullptr, stage_sd_[0], 4 * m * words);
        a.iters = st.route(iters ? iters + done : nullptr, stage_sd_[1], 4 * m);
        a.weight = st.route(weight ? weight + done : nullptr, stage_sd_[2], 4 * m);
        a.first_frame = spec->first_frame + done;
        a.n = m;
        check(launch_bit_flip(a, s), "bit_flip_batch");
        st.flush(s, &pin_out_);
    }
}

// ---------------------------------------------------------------------------------------------
// Min-sum with memory, run as a relay of legs, toward a given syndrome (kernels_relay_decode.hip)
// form 2 (a wave per frame) where four frames fit the CU's LDS and neither side of the code has more nodes than
// kRelayWaveNodes.  Measured on toric codes: form 2 over form 1 is 1.76 x at 72 columns, 1.12 x at
// 288, 0.90 x at 512, 0.99 x at 800, and 0.40 x on h.txt (1152 x 1024); the rule sits halfway between the last size at which
// form 2 won and the first at which it lost
static constexpr int kRelayWaveNodes = 384;

int Engine::relay_form()
{
    if (relay_decode_lds_bytes(kRelayFormWave) < 0)
        return kRelayFormGroup;
    return plan_.nc <= kRelayWaveNodes && plan_.mc <= kRelayWaveNodes ? kRelayFormWave : kRelayFormGroup;
}

int64_t Engine::relay_decode_lds_bytes(int form)
{
    if (form < 0 || form > kRelayFormWave || syndrome_decode_lds_bytes() < 0) // (the codes of syndrome_decode_batch)
        return -1;
    const size_t bytes =
        ldpc_amd::relay_decode_lds_bytes(qms_plan().slots, static_cast<size_t>(plan_.nc), static_cast<size_t>(plan_.mc));
    if (form == 0)
        return bytes <= kCuLdsBytes ? static_cast<int64_t>(bytes) : -1; // (one of the two forms takes it)
    return bytes * (form == kRelayFormWave ? kRelayWaveFrames : 1) <= kCuLdsBytes ? static_cast<int64_t>(bytes) : -1;
}

std::string Engine::relay_decode_refusal(const RelayDecodeSpec *spec, int llr_type, int syndrome_format)
{
    const char *entry = "ldpc_hip_relay_decode_batch";
    const std::string who = std::string(entry) + ": ";
    if (!spec)
        return who + "null parameters";
    if (spec->legs < 1 || spec->legs > 256)
        return who + "legs " + std::to_string(spec->legs) + " is outside 1..256";
    if (spec->first_iterations < 1 || spec->first_iterations > 0xFFFFu)
        return who + "first_iterations " + std::to_string(spec->first_iterations) + " is outside 1..65535";
    if (spec->leg_iterations < 1 || spec->leg_iterations > 0xFFFFu)
        return who + "leg_iterations " + std::to_string(spec->leg_iterations) + " is outside 1..65535";
    if (spec->stop_after < 1 || spec->stop_after > spec->legs)
        return who + "stop_after " + std::to_string(spec->stop_after) + " is outside 1..legs";
    if (spec->q_bits < 2 || spec->q_bits > 8)
        return who + "q_bits " + std::to_string(spec->q_bits) + " is outside 2..8";
    if (!(spec->step > 0.0) || spec->step < 0x1p-20 || spec->step > 0x1p20) // (a NaN fails the first)
        return who + "the step must lie in [2^-20, 2^20]";
    if (!(spec->scale > 0.0) || spec->scale > 1.0)
        return who + "the scale must lie in (0, 1]";
    if (!(spec->offset >= 0.0) || spec->offset > 1e6)
        return who + "the offset must lie in [0, 1e6]";
    if (spec->form < 0 || spec->form > kRelayFormWave)
        return who + "form " + std::to_string(spec->form) + " is outside 0..2";
    if (spec->flags & ~kSyndromeSharedLlr)
        return who + "unknown flag bits " + std::to_string(spec->flags & ~kSyndromeSharedLlr);
    if (llr_type_bytes(llr_type) == 0)
        return who + "unknown LLR type " + std::to_string(llr_type) + " (0 = binary64, 1 = binary32, 2 = binary16, 3 = int8)";
    if (std::string why = bits_format_refusal(entry, "syndrome", syndrome_format); !why.empty())
        return why;
    if (relay_decode_lds_bytes(0) < 0)
        return who + "the code of " + std::to_string(plan_.mc) + " x " + std::to_string(plan_.nc) +
               " is not taken: more than 65 535 columns, a check node with fewer than two entries, or a frame beyond the 160 KB of LDS "
               "of a CU (ldpc_hip_relay_decode_lds_bytes; there is no other kernel)";
    if (relay_decode_lds_bytes(spec->form) < 0)
        return who + "form " + std::to_string(spec->form) + " does not fit the code of " + std::to_string(plan_.mc) + " x " +
               std::to_string(plan_.nc) + ": four frames exceed the 160 KB of LDS of a CU (ldpc_hip_relay_decode_lds_bytes)";
    return "";
}

void Engine::relay_decode_batch(const RelayDecodeSpec *spec, uint64_t n, const void *llr, int llr_type, const void *syndrome,
                                int syndrome_format, const int8_t *gamma, uint32_t *hard_bits, uint32_t *iters, uint32_t *weight,
                                uint32_t *solutions, uint32_t *best_leg, uint32_t *cost, void *stream)
{
    if (const std::string why = relay_decode_refusal(spec, llr_type, syndrome_format); !why.empty())
        throw std::runtime_error(why);
    if (n && !llr)
        throw std::runtime_error("ldpc_hip_relay_decode_batch: null llr");
    if (n == 0 || (!hard_bits && !iters && !weight && !solutions && !best_leg && !cost))
        return;
    upload_plan();
    upload_qms_plan();
    if (!sd_cn_row_)
        sd_cn_row_ = static_cast<const uint32_t *>(upload_table(plan_.cn_rank_row.data(), plan_.cn_rank_row.size() * 4, "check node order"));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t nc = static_cast<uint64_t>(plan_.nc), mc = static_cast<uint64_t>(plan_.mc), words = (nc + 31) / 32;
    const bool shared = (spec->flags & kSyndromeSharedLlr) != 0;
    RelayDecodeArgs a{};
    a.nc = static_cast<uint32_t>(nc), a.mc = static_cast<uint32_t>(mc), a.words = static_cast<uint32_t>(words);
    a.syn_words = static_cast<uint32_t>((mc + 31) / 32);
    a.legs = spec->legs, a.first_iterations = spec->first_iterations, a.leg_iterations = spec->leg_iterations;
    a.stop_after = spec->stop_after;
    a.form = spec->form ? spec->form : relay_form();
    a.llr_type = llr_type, a.syndrome_format = syndrome_format, a.shared_llr = shared ? 1 : 0;
    {
        const QmsArgs q = quantizer_args<QmsArgs>(spec->step, spec->q_bits, spec->scale, spec->offset); // (the same host routine)
        a.qmax = q.qmax, a.inv = q.inv;
        std::memcpy(a.lut, q.lut, sizeof a.lut);
    }
    a.frame_bytes = static_cast<uint32_t>(relay_decode_lds_bytes(a.form));
    a.col_rank = dev_.col_rank, a.rank_col = dev_.rank_col, a.cn_row = sd_cn_row_;
    a.gamma = gamma ? static_cast<const int8_t *>(stage_input(gamma, static_cast<size_t>(spec->legs) * nc, stage_relay_gamma_, stream)) : nullptr;
    const size_t elem = llr_type_bytes(llr_type), in_row = elem * nc, syn_row = bits_row_bytes(syndrome_format, mc);
    DeviceBuffer &llr_stage = llr_type == kLlrF64 ? stage_in_ : stage_typed_;
    if (shared) // one row for every frame: staged once
        a.llr = stage_input(llr, in_row, llr_stage, stream);
    const uint64_t sub = std::max<uint64_t>(gf2_sub_batch() / elem, 1); // (elements of up to 8 bytes, not bits)
    for (uint64_t done = 0; done < n; done += sub)
    {
        const uint64_t m = std::min(sub, n - done);
        if (!shared)
            a.llr = stage_input(static_cast<const char *>(llr) + in_row * done, in_row * m, llr_stage, stream);
        a.syndrome = syndrome ? stage_input(static_cast<const char *>(syndrome) + syn_row * done, syn_row * m, stage_in_b_, stream) : nullptr;
        OutStage st;
        a.hard_bits = st.route(hard_bits ? hard_bits + done * words : nullptr, stage_sd_[0], 4 * m * words);
        a.iters = st.route(iters ? iters + done : nullptr, stage_sd_[1], 4 * m);
        a.weight = st.route(weight ? weight + done : nullptr, stage_sd_[2], 4 * m);
        a.solutions = st.route(solutions ? solutions + done : nullptr, stage_relay_[0], 4 * m);
        a.best_leg = st.route(best_leg ? best_leg + done : nullptr, stage_relay_[1], 4 * m);
        a.cost = st.route(cost ? cost + done : nullptr, stage_relay_[2], 4 * m);
        a.n = m;
        check(launch_relay_decode(a, dev_qms_, s), "relay_decode_batch");
        st.flush(s, &pin_out_);
    }
}

void Engine::stream_rewind_encoder(uint64_t frames_back, void *stream)
{
    if (!code_->has_G() || frames_back == 0 || counter_) // (counter-based noise: a codeword depends on its frame index alone)
        return;
    if (frames_back > last_enc_n_)
        throw std::runtime_error("stream_rewind_encoder: more frames than the last batch held");
    bind_device();
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nc = plan_.nc;
    const uint8_t *src = frames_back == last_enc_n_
                             ? static_cast<const uint8_t *>(cw_before_.get())
                             : static_cast<const uint8_t *>(cw_frames_.get()) + (last_enc_n_ - frames_back - 1) * nc;
    check(hipMemcpyAsync(cw_run_.get(), src, nc, hipMemcpyDeviceToDevice, s), "codeword rewind");
    info_pos_ -= frames_back * static_cast<uint64_t>(code_->kc());
    last_enc_n_ = 0;
}

// ---------------------------------------------------------------------------------------------
void Engine::stream_begin(int channel, uint64_t seed, double x, bool fresh)
{
    if (channel != kAwgn && channel != kBsc && channel != kBec)
        throw std::runtime_error("No channel selected.");
    chan_ = channel;
    counter_ = noise_mode == 1;
    ctr_seed_ = seed;
    // jump-ahead in four thread groups where its latency counts: the erasure channel (its bit-sliced decoder leaves the noise
    // chain on the critical path) and beside the register-resident decoders (rng_kernels.hip, mt_jump_kernel)
    noise_.st.set_jump_groups(channel == kBec || register_resident() ? 4 : 1);
    x_ = x;
    frame_pos_ = 0;
    raw_next_ = 0;
    cur_pair_ = cur_chunk_ = cur_k_ = 0;
    small_cache_.valid = false;
    sh_chunk_ = sh_pairs_ = 0;
    stream_mode_ = 0;
    noise_.reset(seed);
    if (fresh || info_.seed() != (seed << 1))
    {
        info_.reset(seed << 1); // channel.cpp:11
        info_pos_ = 0;
        cw_run_valid_ = false;
    }
    if (channel == kAwgn)
    {
        sigma2_ = std::pow(10, -x / 10); // channel.cpp:39
        sigma_ = std::sqrt(sigma2_);
    }
    else
        delta_ = std::log((1 - x) / x); // channel.cpp:139
}

void Engine::ensure_rng_stream()
{
    if (rng_stream_)
        return;
    // non-blocking: no implicit ordering with the caller's (possibly default) stream
    hipStream_t rs;
    check(hipStreamCreateWithFlags(&rs, hipStreamNonBlocking), "hipStreamCreate");
    rng_stream_ = rs;
    for (int i = 0; i < 2; ++i)
    {
        hipEvent_t e0, e1;
        check(hipEventCreateWithFlags(&e0, hipEventDisableTiming), "hipEventCreate");
        check(hipEventCreateWithFlags(&e1, hipEventDisableTiming), "hipEventCreate");
        ev_pairs_ready_[i] = e0, ev_pairs_free_[i] = e1;
    }
}

const uint64_t *Engine::noise_raw_async(uint64_t first, uint64_t count, void *stream, int &buffer)
{
    ensure_rng_stream();
    hipStream_t s = static_cast<hipStream_t>(rng_stream_), user = static_cast<hipStream_t>(stream);
    const int buf = pp_;
    pp_ ^= 1;
    // the launch that last read this buffer (two batches ago) must be done before it is refilled
    if (pairs_in_use_[buf])
        check(hipStreamWaitEvent(s, static_cast<hipEvent_t>(ev_pairs_free_[buf]), 0), "wait raw free");
    prof_mark(1, s);
    const uint64_t *raw = noise_.generate(first, count, s, buf);
    prof_mark(1, s);
    check(hipEventRecord(static_cast<hipEvent_t>(ev_pairs_ready_[buf]), s), "event");
    check(hipStreamWaitEvent(user, static_cast<hipEvent_t>(ev_pairs_ready_[buf]), 0), "wait raw ready");
    buffer = buf;
    return raw;
}

void Engine::noise_raw_release(int buffer, void *stream)
{
    check(hipEventRecord(static_cast<hipEvent_t>(ev_pairs_free_[buffer]), static_cast<hipStream_t>(stream)), "event");
    pairs_in_use_[buffer] = true;
}

// One pass of the noise generator on the side stream: `full` whole chunks from `chunk` on (+ a prefix of last_blocks twist
// blocks of the chunk after them) -> normals in the slabs of buffer `buf`, their counts, the slab table, and where the
// consumer stands afterwards.  Chunk start states: the ring (one rank reading front to back) or the strided table (sharded).
Engine::NoisePass Engine::noise_pass(uint64_t chunk, uint32_t full, uint32_t last_blocks, uint32_t n_piece, uint64_t need, uint64_t target,
                                     int buf, bool write_normals, bool strided, uint64_t stride)
{
    hipStream_t s = static_cast<hipStream_t>(rng_stream_);
    MtDevice &st = noise_.st;
    NoisePass np;
    np.n_slabs = full + (last_blocks ? 1 : 0);
    if (np.n_slabs == 0)
        throw std::runtime_error("noise generator: empty pass");
    if (np.n_slabs > (strided ? StridedTable::kMaxRows : StateRing::kWindow))
        throw std::runtime_error("noise generator: batch spans more chunks than the state table holds");
    const uint64_t slab_words = 2 * st.chunk_trials();
    NormalsArgs na{};
    if (strided)
    {
        na.ring = st.ensure_strided(chunk, np.n_slabs, stride, s);
        na.ring_rows = MtDevice::strided_rows();
        na.first_row = 0;
    }
    else
    {
        na.first_row = st.ensure_ring(chunk, chunk + np.n_slabs, s);
        na.ring = st.ring();
        na.ring_rows = MtDevice::ring_rows();
    }
    // (two slabs of slack: the number of chunks a batch spans varies by one, and growing a buffer means freeing it first)
    np.slabs = write_normals ? static_cast<uint64_t *>(slabs_[buf].reserve(8 * slab_words * (np.n_slabs + 2))) : nullptr;
    // (a counting pass must not touch the slab table a decode launch in flight may still read)
    np.cum = static_cast<uint64_t *>((write_normals ? slab_cum_[buf] : nz_cum_skip_).reserve(8 * (static_cast<size_t>(np.n_slabs) + 8)));
    uint32_t *counts = static_cast<uint32_t *>(nz_counts_.reserve(4 * static_cast<size_t>(np.n_slabs)));
    NormalsResult *res = static_cast<NormalsResult *>(nz_result_.reserve(sizeof(NormalsResult)));
    na.slabs = np.slabs;
    na.slab_words = slab_words;
    na.counts = counts;
    na.write_normals = write_normals ? 1 : 0;
    na.locate_chunk = 0xFFFFFFFFu;
    na.pack = noise_.pack();
    na.raw = static_cast<uint64_t *>(nz_raw_.reserve(8 * st.chunk_words() * (np.n_slabs + 2)));
    na.lookback = static_cast<uint64_t *>(nz_lookback_.reserve(8 * normals_lookback_words(np.n_slabs + 2, st.chunk_blocks())));
    na.n_chunks = np.n_slabs;
    na.blocks = st.chunk_blocks();
    na.last_blocks = last_blocks ? last_blocks : st.chunk_blocks(); // (the prefix chunk rides in the same two launches)
    check(launch_mt_normals(na, s), "mt_normals");
    check(launch_normals_finish(counts, np.n_slabs, n_piece, full, need, target, np.cum, res, s), "normals_finish");
    check(hipMemcpyAsync(&np.res, res, sizeof np.res, hipMemcpyDeviceToHost, s), "noise result");
    const auto t0 = std::chrono::steady_clock::now();
    check(hipStreamSynchronize(s), "sync"); // waits for the noise-stream kernels only, not for the caller's decode
    host_ms_[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), ++host_n_[1];
    return np;
}

void Engine::fill_slab_args(DecodeArgs &a, const NoisePass &np, uint64_t pair_origin, int buf) const
{
    a.pairs = np.slabs;
    a.slab_cum = np.cum;
    a.slab_words = 2 * noise_.st.chunk_trials();
    a.n_slabs = np.n_slabs;
    a.slab_pairs_inv = static_cast<float>(1.0 / (static_cast<double>(noise_.st.chunk_trials()) * 0.7853981633974483));
    a.pair_origin = pair_origin;
    a.sigma = sigma_, a.sigma2 = sigma2_, a.inv_sigma2 = 1.0 / sigma2_;
    a.shorten_llr = 99999.9; // channel.cpp:83
    a.pairs_buffer = buf;
}

// The normals of frames [frame_pos_, frame_pos_ + n): normal g is element g & 1 of accepted pair g >> 1.
void Engine::awgn_prepare(uint64_t n, DecodeArgs &a, void *stream, bool write_normals)
{
    hipStream_t user = static_cast<hipStream_t>(stream);
    ensure_rng_stream();
    hipStream_t s = static_cast<hipStream_t>(rng_stream_);
    const uint64_t nct = static_cast<uint64_t>(plan_.nct);
    const uint64_t g0 = frame_pos_ * nct, g1 = g0 + n * nct; // normals [g0, g1)
    const uint64_t q0 = g0 >> 1, q1 = (g1 - 1) >> 1, qn = g1 >> 1;
    if (q0 != cur_pair_)
        throw std::runtime_error("noise stream out of step");
    // pairs that must exist from the start of chunk cur_chunk_ on / list index of the first pair the NEXT batch needs
    const uint64_t need = cur_k_ + (q1 - q0 + 1), target = cur_k_ + (qn - q0);
    if (write_normals && small_cache_.valid && small_cache_.chunk == cur_chunk_ && need <= small_cache_.np.res.total &&
        target < small_cache_.np.res.total)
    {
        // (the slab was complete when the pass that made it returned, and the decode launches that read it since are
        // ordered on the caller's stream by the events of run_decode as for any batch)
        check(hipStreamWaitEvent(user, static_cast<hipEvent_t>(ev_pairs_ready_[small_cache_.buf]), 0), "wait pairs ready");
        fill_slab_args(a, small_cache_.np, q0 - cur_k_, small_cache_.buf);
        a.normal_base = g0;
        cur_k_ = target;
        cur_pair_ = qn;
        return;
    }
    const int buf = pp_;
    if (write_normals)
    {
        pp_ ^= 1;
        if (small_cache_.buf == buf)
            small_cache_.valid = false;
        // the decode kernel that last read this slab buffer (two batches ago) must be done before it is refilled
        if (pairs_in_use_[buf])
            check(hipStreamWaitEvent(s, static_cast<hipEvent_t>(ev_pairs_free_[buf]), 0), "wait pairs free");
    }
    const uint64_t ct = noise_.st.chunk_trials();
    double trials = static_cast<double>(need) * 1.2732395447351628 + 8.0 * std::sqrt(static_cast<double>(need)) + 256;
    // a small request: two dozen frames further than asked (a fraction of the prefix's serial chain), for the requests
    // that are likely to follow (small_cache_)
    const bool small = write_normals && n <= 16;
    if (small)
        trials += 24.0 * static_cast<double>(nct / 2 + 1) * 1.2732395447351628;
    NoisePass np;
    prof_mark(1, s);
    for (;;)
    {
        const uint64_t t = static_cast<uint64_t>(trials);
        uint64_t full = t / ct;
        uint32_t last_blocks = static_cast<uint32_t>((t - full * ct + kBlockTrials - 1) / kBlockTrials);
        if (last_blocks >= noise_.st.chunk_blocks())
            ++full, last_blocks = 0;
        np = noise_pass(cur_chunk_, static_cast<uint32_t>(full), last_blocks, static_cast<uint32_t>(full + (last_blocks ? 1 : 0)), need, target,
                        buf, write_normals, false, 0);
        if (np.res.enough)
            break;
        trials += trials / 8 + 4096; // vanishingly rare: take a longer look at the same stream
    }
    prof_mark(1, s);
    if (write_normals)
    {
        check(hipEventRecord(static_cast<hipEvent_t>(ev_pairs_ready_[buf]), s), "event");
        check(hipStreamWaitEvent(user, static_cast<hipEvent_t>(ev_pairs_ready_[buf]), 0), "wait pairs ready");
        fill_slab_args(a, np, q0 - cur_k_, buf);
        a.normal_base = g0;
    }
    if (write_normals)
    {
        small_cache_.valid = small && np.n_slabs == 1 && np.res.next_slab == 0;
        small_cache_.chunk = cur_chunk_, small_cache_.buf = buf, small_cache_.np = np;
    }
    cur_chunk_ += np.res.next_slab;
    cur_k_ = np.res.next_k;
    cur_pair_ = qn;
    // the chunk start states of the next batch but one, now: their jump-ahead chain then runs beside the next batch's
    // generator chain (both hide under decode kernels whose waves outrank them, kernels.hip), not in front of it
    noise_.st.prefetch_ring(cur_chunk_ + 2 * (static_cast<uint64_t>(np.n_slabs) + 2));
}

// raw 64-bit draws consumed from the noise stream since stream_begin (what orc_chan_raw_draws counts)
uint64_t Engine::stream_raw_draws()
{
    if (counter_)
        throw std::runtime_error("stream_raw_draws: counter-based noise draws from no stream (ldpc_hip_set_noise)");
    if (chan_ != kAwgn)
        return raw_next_;
    if (stream_mode_ == 2)
        return sh_chunk_ * noise_.st.chunk_words();
    const uint64_t nct = static_cast<uint64_t>(plan_.nct);
    const uint64_t g1 = frame_pos_ * nct;
    if (g1 == 0)
        return 0;
    // the last pair the stream has drawn: (g1 - 1) >> 1.  cur_* describe pair g1 >> 1: the same pair (its second normal is
    // still saved) when g1 is odd, the pair before it otherwise — which may be the last accepted pair of the previous chunk.
    bind_device();
    ensure_rng_stream();
    hipStream_t s = static_cast<hipStream_t>(rng_stream_);
    uint64_t chunk = cur_chunk_;
    uint32_t rank = static_cast<uint32_t>(cur_k_);
    if ((g1 & 1) == 0)
    {
        if (cur_k_ > 0)
            --rank;
        else
            --chunk, rank = 0xFFFFFFFFu;
    }
    MtDevice &st = noise_.st;
    NormalsArgs na{};
    na.first_row = st.ensure_ring(chunk, chunk + 1, s);
    na.ring = st.ring();
    na.ring_rows = MtDevice::ring_rows();
    na.n_chunks = 1;
    na.blocks = na.last_blocks = st.chunk_blocks();
    na.slab_words = 2 * st.chunk_trials();
    na.counts = static_cast<uint32_t *>(nz_counts_.reserve(4));
    na.write_normals = 0;
    na.locate_chunk = 0;
    na.locate_rank = rank;
    na.locate_out = static_cast<uint64_t *>(nz_locate_.reserve(8));
    na.pack = 1;
    na.raw = static_cast<uint64_t *>(nz_raw_.reserve(8 * st.chunk_words()));
    na.lookback = static_cast<uint64_t *>(nz_lookback_.reserve(8 * normals_lookback_words(1, st.chunk_blocks())));
    const uint64_t none = rank == 0xFFFFFFFFu ? 0 : ~0ull; // ("last pair": a running maximum over the chunk's workgroups)
    uint64_t t = none;
    check(hipMemcpyAsync(na.locate_out, &t, 8, hipMemcpyHostToDevice, s), "locate");
    check(hipStreamSynchronize(s), "sync");
    check(launch_mt_normals(na, s), "mt_normals (locate)");
    check(hipMemcpyAsync(&t, na.locate_out, 8, hipMemcpyDeviceToHost, s), "locate");
    check(hipStreamSynchronize(s), "sync");
    if (rank != 0xFFFFFFFFu && t == none)
        throw std::runtime_error("noise stream position not found");
    return 2 * (chunk * st.chunk_trials() + t + 1);
}

void Engine::stream_skip(uint64_t n_frames, void *stream)
{
    if (!chan_)
        throw std::runtime_error("stream_begin() has not been called");
    if (stream_mode_ == 2)
        throw std::runtime_error("stream_skip after stream_decode_sharded on the same stream: call stream_begin first");
    stream_mode_ = 1;
    if (counter_) // (a frame's noise and codeword depend on its index alone)
    {
        frame_pos_ += n_frames;
        return;
    }
    upload_plan();
    const uint64_t nct = static_cast<uint64_t>(plan_.nct);
    while (n_frames)
    {
        const uint64_t n = std::min<uint64_t>(n_frames, max_sub_batch());
        encode_frames(n, false, stream);
        if (chan_ == kAwgn)
        {
            DecodeArgs a{};
            awgn_prepare(n, a, stream, /*write_normals=*/false);
        }
        else
            raw_next_ += n * nct;
        frame_pos_ += n;
        n_frames -= n;
    }
}

void Engine::stream_decode(const DecParams &p, uint64_t n_frames, const BatchOut &out, void *stream)
{
    if (!chan_)
        throw std::runtime_error("stream_begin() has not been called");
    if (n_frames == 0)
        return;
    if (stream_mode_ == 2)
        throw std::runtime_error("stream_decode after stream_decode_sharded on the same stream: call stream_begin first");
    stream_mode_ = 1;
    upload_plan();
    const uint64_t nct = static_cast<uint64_t>(plan_.nct), nc = static_cast<uint64_t>(plan_.nc);
    const uint64_t sub = max_sub_batch();
    uint64_t done = 0;
    while (done < n_frames)
    {
        const uint64_t n = std::min<uint64_t>(n_frames - done, sub);
        const BatchOut o = out.at(done, nc);
        if (counter_)
        {
            run_counter(p, o, frame_pos_, n, stream);
            frame_pos_ += n;
            done += n;
            continue;
        }
        const uint8_t *cw = encode_frames(n, true, stream);
        DecodeArgs a{};
        a.codeword = cw;
        if (chan_ == kAwgn)
        {
            a.mode = kModeAwgn;
            awgn_prepare(n, a, stream);
            run_decode(a, p, o, n, stream);
        }
        else
        {
            if (chan_ == kBsc)
                run_bsc(a, p, o, n, raw_next_, stream);
            else
                run_bec(p, o, n, cw, raw_next_, stream);
            raw_next_ += n * nct;
        }
        frame_pos_ += n;
        done += n;
    }
}

// ---------------------------------------------------------------------------------------------
// Geometry of a sharded AWGN step of about target_frames frames over `world` ranks: every rank's piece is `m` whole
// generator chunks (so that its chunk start states are the previous step's advanced by ONE polynomial, world * m chunks),
// followed by a margin of one frame's worth of trials from the next chunk.
namespace
{
struct ShardGeometry
{
    uint32_t m;             // chunks per piece
    uint32_t margin_blocks; // twist blocks of the chunk after the piece that are generated as well
};
ShardGeometry shard_geometry(uint64_t target_frames, int world, uint64_t nct, uint64_t chunk_trials, uint32_t chunk_blocks)
{
    const double pairs_per_rank = static_cast<double>(std::max<uint64_t>(target_frames, 1)) * static_cast<double>(nct) / 2.0 / world;
    const double chunks = pairs_per_rank * 1.2732395447351628 / static_cast<double>(chunk_trials);
    ShardGeometry g;
    g.m = static_cast<uint32_t>(std::clamp<double>(std::floor(chunks + 0.5), 1.0, static_cast<double>(StridedTable::kMaxRows - 1)));
    // the pairs of one frame beyond the piece (the last frame a rank owns may end in its neighbour's piece): twice the
    // expected trials plus 8192, in whole blocks
    const uint64_t margin_trials = (nct / 2 + 2) * 2 + 8192;
    g.margin_blocks = static_cast<uint32_t>(std::min<uint64_t>((margin_trials + kBlockTrials - 1) / kBlockTrials, chunk_blocks));
    return g;
}
} // namespace

uint64_t Engine::shard_capacity(uint64_t target_frames, int world) const
{
    world = std::max(world, 1);
    const uint64_t nct = static_cast<uint64_t>(plan_.nct);
    const uint64_t even = (std::max<uint64_t>(target_frames, 1) + world - 1) / world; // BSC / BEC: even split
    if (counter_)
        return even; // (counter-based noise: every channel splits evenly)
    // AWGN: a frame belongs to the rank whose piece holds its first pair; a piece of m chunks holds at most m * chunk_trials
    // pairs (every trial accepted), i.e. at most that many / (nct / 2) frame starts — a bound, not a statistical estimate
    const ShardGeometry g = shard_geometry(target_frames, world, nct, noise_.st.chunk_trials(), noise_.st.chunk_blocks());
    const uint64_t awgn = (2 * static_cast<uint64_t>(g.m) * noise_.st.chunk_trials() + nct - 1) / nct + 2;
    return std::max(even, awgn);
}

void Engine::encoder_snapshot(void *stream)
{
    if (!code_->has_G() || counter_)
        return;
    bind_device();
    const size_t nc = plan_.nc;
    enc_snap_pos_ = info_pos_;
    enc_snap_valid_ = cw_run_valid_;
    if (cw_run_valid_)
        check(hipMemcpyAsync(enc_snap_.reserve(nc), cw_run_.get(), nc, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)),
              "encoder snapshot");
}

void Engine::encoder_restore_and_skip(uint64_t frames, void *stream)
{
    if (!code_->has_G() || counter_)
        return;
    bind_device();
    const size_t nc = plan_.nc;
    info_pos_ = enc_snap_pos_;
    cw_run_valid_ = enc_snap_valid_;
    if (enc_snap_valid_)
        check(hipMemcpyAsync(cw_run_.reserve(nc), enc_snap_.get(), nc, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)),
              "encoder restore");
    for (uint64_t left = frames; left;)
    {
        const uint64_t n = std::min<uint64_t>(left, 1u << 17);
        encode_frames(n, false, stream);
        left -= n;
    }
    last_enc_n_ = 0;
}

Engine::ShardStep Engine::stream_decode_sharded(Comm &comm, const DecParams &p, uint64_t target_frames, const BatchOut &out,
                                                void *stream, const std::string *failed_before)
{
    // (argument errors: the same on every rank, thrown before anything is exchanged)
    if (!chan_)
        throw std::runtime_error("stream_begin() has not been called");
    const int R = comm.world(), r = comm.rank();
    const uint64_t nct = static_cast<uint64_t>(plan_.nct), cap = shard_capacity(target_frames, R);
    target_frames = std::max<uint64_t>(target_frames, 1);
    if (stream_mode_ == 1)
        throw std::runtime_error("stream_decode_sharded after stream_decode on the same stream: call stream_begin first");
    stream_mode_ = 2;
    if ((chan_ != kAwgn || counter_) && !failed_before)
        upload_plan();
    ShardStep st;
    st.step_first = frame_pos_;
    DecodeArgs a{};
    if (counter_)
    {
        // counter-based noise: an even split of the step, nothing exchanged (the encoder's codewords included)
        if (failed_before)
            throw std::runtime_error(*failed_before);
        if (cap > max_sub_batch())
            throw std::runtime_error("sharded step too large for one launch per rank");
        st.step_frames = target_frames;
        const uint64_t base = target_frames / R, extra = target_frames % R;
        st.n = base + (static_cast<uint64_t>(r) < extra ? 1 : 0);
        st.first = st.step_first + base * r + std::min<uint64_t>(r, extra);
        if (st.n)
            run_counter(p, out, st.first, st.n, stream);
        frame_pos_ = st.step_first + st.step_frames;
        return st;
    }
    if (chan_ == kAwgn)
    {
        // The step: world * m whole chunks of the raw stream.  Rank r generates chunks [base + r m, base + (r+1) m) and the
        // head of the next one, counts its accepted pairs, and ONE all-gather of {pairs in the piece, pairs incl. the
        // margin, status} places every piece in the pair sequence.  Every rank can then evaluate every rank's conditions:
        // a failure anywhere makes all ranks throw together instead of leaving the others in the next collective.
        const ShardGeometry g = shard_geometry(target_frames, R, nct, noise_.st.chunk_trials(), noise_.st.chunk_blocks());
        const uint64_t stride = static_cast<uint64_t>(R) * g.m;
        uint64_t send[3] = {0, 0, 0};
        NoisePass np;
        std::string local_error;
        int buf = -1;
        try
        {
            // (a caller whose own preparation failed on this rank — the simulation loop's encoder snapshot — still has to
            // take part in the exchange below, or the other ranks wait in it for ever: it enters with the failure in hand)
            if (failed_before)
                throw std::runtime_error(*failed_before);
            if (cap > max_sub_batch())
                throw std::runtime_error("sharded step too large for one launch per rank");
            upload_plan(); // (the first touch of the GPU: a rank without a usable device fails here, inside the guarded part)
            ensure_rng_stream();
            hipStream_t s = static_cast<hipStream_t>(rng_stream_);
            buf = pp_;
            pp_ ^= 1;
            if (small_cache_.buf == buf)
                small_cache_.valid = false;
            if (pairs_in_use_[buf])
                check(hipStreamWaitEvent(s, static_cast<hipEvent_t>(ev_pairs_free_[buf]), 0), "wait pairs free");
            prof_mark(1, s);
            np = noise_pass(sh_chunk_ + static_cast<uint64_t>(r) * g.m, g.m, g.margin_blocks, g.m, 0, 0, buf, true, true, stride);
            prof_mark(1, s);
            send[0] = np.res.piece, send[1] = np.res.total;
            // the chunk start states of the next step but one, now: their jump-ahead chain has a whole step to run, on a stream
            // of its own, and every step's generator chain starts at once (MtDevice::prefetch_strided)
            noise_.st.prefetch_strided();
        }
        catch (const std::exception &e)
        {
            local_error = e.what();
            send[2] = 1;
        }
        std::vector<uint64_t> all(3 * static_cast<size_t>(R));
        const auto t0 = std::chrono::steady_clock::now();
        comm.all_gather(send, all.data(), sizeof send);
        host_ms_[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), ++host_n_[0];
        const ShardPlacement pl = place_pieces(all.data(), R, r, sh_pairs_, frame_pos_, nct, cap, local_error); // (shard_place.hpp)
        st.first = pl.first, st.n = pl.n, st.step_frames = pl.step_frames;
        hipStream_t s = static_cast<hipStream_t>(rng_stream_), user = static_cast<hipStream_t>(stream);
        check(hipEventRecord(static_cast<hipEvent_t>(ev_pairs_ready_[buf]), s), "event");
        check(hipStreamWaitEvent(user, static_cast<hipEvent_t>(ev_pairs_ready_[buf]), 0), "wait pairs ready");
        a.mode = kModeAwgn;
        fill_slab_args(a, np, pl.pair_start, buf);
        a.normal_base = st.first * nct;
        sh_pairs_ = pl.pairs_after;
        sh_chunk_ += stride;
    }
    else
    {
        if (failed_before) // (no exchange inside a BSC / BEC step: the caller's own exchange carries the failure)
            throw std::runtime_error(*failed_before);
        if (cap > max_sub_batch())
            throw std::runtime_error("sharded step too large for one launch per rank");
        st.step_frames = target_frames;
        const uint64_t base = target_frames / R, extra = target_frames % R;
        st.n = base + (static_cast<uint64_t>(r) < extra ? 1 : 0);
        st.first = st.step_first + base * r + std::min<uint64_t>(r, extra);
    }
    // encoder: a rank draws the info words of its own frames only; one all-gather of the ranks' info-word sums (ceil(kc / 64)
    // words) gives each the word its prefixes start from and all of them the codeword accumulated over the step
    const uint8_t *cw = nullptr;
    if (code_->has_G())
    {
        cw = encode_frames_sharded(comm, st.first - st.step_first, st.n, st.step_frames, stream);
        last_enc_n_ = 0;
    }
    if (st.n)
    {
        if (chan_ == kAwgn)
        {
            a.codeword = cw;
            run_decode(a, p, out, st.n, stream);
        }
        else if (chan_ == kBsc)
        {
            a.codeword = cw;
            run_bsc(a, p, out, st.n, st.first * nct, stream);
        }
        else
            run_bec(p, out, st.n, cw, st.first * nct, stream);
    }
    else if (chan_ == kAwgn && a.pairs_buffer >= 0)
        pairs_in_use_[a.pairs_buffer] = false;
    if (chan_ != kAwgn)
        raw_next_ = (st.step_first + st.step_frames) * nct;
    frame_pos_ = st.step_first + st.step_frames;
    return st;
}

} // namespace ldpc_amd
