// sim_kernels.hip — what the simulation loop launches around the decoder: the GF(2) encoder (EncodeArgs, kernels.hpp) and
// the five counters of a batch.
//
// Reference semantics restated here (file:line in heat1q/libldpc):
//   encoder                src/sim/channel.cpp:44-60, src/core/sparse.h:163-172
//   bit-error count        src/sim/ldpcsim.cpp:184-188
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "kernels.hpp"

namespace ldpc_amd
{

namespace
{

// ---------------------------------------------------------------------------------------------
// encoder (see EncodeArgs)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void encode_info_kernel(const EncodeArgs a)
{
    // one thread per (frame, word): 64 bernoulli(0.5) draws -> one packed word
    const uint64_t gid = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (gid >= a.n_frames * static_cast<uint64_t>(a.words))
        return;
    const uint64_t f = gid / a.words;
    const int w = static_cast<int>(gid % a.words);
    const uint64_t *raw = a.info_raw + f * static_cast<uint64_t>(a.kc) + 64 * w;
    const int nb = min(64, a.kc - 64 * w);
    uint64_t bits = 0;
    for (int i = 0; i < nb; ++i)
        bits |= static_cast<uint64_t>(canonical(raw[i]) < 0.5) << i;
    a.prefix[gid] = bits;
}

// running XOR over frames, one workgroup per packed word column
__global__ __launch_bounds__(1024) void encode_prefix_kernel(const EncodeArgs a)
{
    __shared__ uint64_t part[1024];
    const int w = blockIdx.x, tid = threadIdx.x;
    const uint64_t per = (a.n_frames + 1023) / 1024;
    const uint64_t lo = min(tid * per, a.n_frames), hi = min(lo + per, a.n_frames);
    uint64_t s = 0;
    for (uint64_t f = lo; f < hi; ++f)
        s ^= a.prefix[f * a.words + w];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1)
    {
        uint64_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] ^= v;
        __syncthreads();
    }
    uint64_t run = tid ? part[tid - 1] : 0;
    for (uint64_t f = lo; f < hi; ++f)
    {
        run ^= a.prefix[f * a.words + w];
        a.prefix[f * a.words + w] = run;
    }
}

// codeword[f][j] = cw_prev[j] ^ parity(prefix_f restricted to the rows of column j of G)
__global__ __launch_bounds__(256) void encode_cw_kernel(const EncodeArgs a, uint64_t first_frame)
{
    extern __shared__ uint64_t pw[];
    const uint64_t f = first_frame + blockIdx.x;
    for (int w = threadIdx.x; w < a.words; w += 256)
        pw[w] = a.prefix[f * a.words + w] ^ (a.base ? a.base[w] : 0ull);
    __syncthreads();
    const bool last = f + 1 == a.n_frames;
    uint8_t *out = a.codeword ? a.codeword + f * a.nc : nullptr;
    for (int j = threadIdx.x; j < a.nc; j += 256)
    {
        uint8_t b = a.cw_prev[j];
        if (j < a.g_cols)
            for (uint32_t p = a.g_col_ptr[j]; p < a.g_col_ptr[j + 1]; ++p)
            {
                uint32_t r = a.g_col_row[p];
                b ^= static_cast<uint8_t>(pw[r >> 6] >> (r & 63) & 1);
            }
        if (out)
            out[j] = b;
        if (last)
            a.cw_last[j] = b;
    }
}

// the same with the columns of G as bit masks (EncodeArgs::g_mask): a workgroup takes kEncFrames consecutive frames, a thread
// keeps the masks of its columns in registers (W words each) and the frames' prefixes arrive as scalars — a codeword bit is
// W ANDs and a population count instead of a walk over the column's entries with a bit test each (the walk: 3.5 ms per
// 65 536 frames of the n = 1024 code, more than the decode launch it feeds)
constexpr int kEncFrames = 32, kEncCols = 8; // columns per thread the kernel provides for: nc <= 256 * kEncCols
template <int W>
__global__ __launch_bounds__(256) void encode_cw_dense_kernel(const EncodeArgs a, uint64_t first_frame, uint64_t n_do)
{
    uint64_t m[kEncCols][W];
    uint8_t prev[kEncCols];
#pragma unroll
    for (int c = 0; c < kEncCols; ++c)
    {
        const int j = threadIdx.x + 256 * c;
        prev[c] = j < a.nc ? a.cw_prev[j] : 0;
#pragma unroll
        for (int w = 0; w < W; ++w)
            m[c][w] = j < a.nc ? a.g_mask[static_cast<size_t>(j) * W + w] : 0;
    }
    uint64_t base[W];
#pragma unroll
    for (int w = 0; w < W; ++w)
        base[w] = a.base ? uniform_table(a.base)[w] : 0ull;
    const uint64_t f0 = first_frame + static_cast<uint64_t>(blockIdx.x) * kEncFrames;
    const auto pre = uniform_table(a.prefix);
    for (int k = 0; k < kEncFrames; ++k)
    {
        const uint64_t f = f0 + k;
        if (f >= first_frame + n_do)
            break;
        uint64_t p[W];
#pragma unroll
        for (int w = 0; w < W; ++w)
            p[w] = pre[f * W + w] ^ base[w];
        const bool last = f + 1 == a.n_frames;
        uint8_t *out = a.codeword ? a.codeword + f * a.nc : nullptr;
#pragma unroll
        for (int c = 0; c < kEncCols; ++c)
        {
            const int j = threadIdx.x + 256 * c;
            if (j >= a.nc)
                break;
            uint64_t x = 0;
#pragma unroll
            for (int w = 0; w < W; ++w)
                x ^= p[w] & m[c][w];
            const uint8_t b = prev[c] ^ static_cast<uint8_t>(__popcll(x) & 1);
            if (out)
                out[j] = b;
            if (last)
                a.cw_last[j] = b;
        }
    }
}

// one workgroup sums the per-frame outputs of a batch (64 K frames: 64 per thread) into the five counters of the
// simulation loop (ldpcsim.cpp:175-200): frames, frame errors, bit errors, iterations, early stops
__global__ __launch_bounds__(1024) void batch_counters_kernel(const uint32_t *iters, const uint32_t *bit_errors, uint64_t n,
                                                              uint32_t max_iters, int early_term, long long *counters)
{
    __shared__ long long part[4][16];
    long long fe = 0, be = 0, it = 0, es = 0;
    auto take = [&](uint32_t b, uint32_t t) { fe += b > 0, be += b, it += t, es += early_term && t < max_iters; };
    // four frames per load, four loads in flight per array: the kernel sits between two batches' decode launches, and 64
    // dependent round trips per thread (one frame per load) were 35 us of every step
    uint64_t done = 0;
    if ((reinterpret_cast<uintptr_t>(iters) | reinterpret_cast<uintptr_t>(bit_errors)) % 16 == 0)
    {
        const uint4 *b4 = reinterpret_cast<const uint4 *>(bit_errors), *t4 = reinterpret_cast<const uint4 *>(iters);
        const uint64_t n4 = n / 4;
        uint64_t i = threadIdx.x;
        for (; i + 3 * 1024 < n4; i += 4 * 1024)
        {
            uint4 b[4], t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                b[k] = b4[i + k * 1024], t[k] = t4[i + k * 1024];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                take(b[k].x, t[k].x), take(b[k].y, t[k].y), take(b[k].z, t[k].z), take(b[k].w, t[k].w);
        }
        for (; i < n4; i += 1024)
        {
            const uint4 b = b4[i], t = t4[i];
            take(b.x, t.x), take(b.y, t.y), take(b.z, t.z), take(b.w, t.w);
        }
        done = n4 * 4;
    }
    for (uint64_t i = done + threadIdx.x; i < n; i += 1024)
        take(bit_errors[i], iters[i]);
    auto wave_total = [](long long v) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            v += __shfl_xor(v, o, 64);
        return v;
    };
    fe = wave_total(fe), be = wave_total(be), it = wave_total(it), es = wave_total(es);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        part[0][wave] = fe, part[1][wave] = be, part[2][wave] = it, part[3][wave] = es;
    __syncthreads();
    if (threadIdx.x < 4)
    {
        long long s = 0;
        for (int w = 0; w < 16; ++w)
            s += part[threadIdx.x][w];
        counters[1 + threadIdx.x] = s;
    }
    if (threadIdx.x == 4)
        counters[0] = static_cast<long long>(n);
}

} // namespace

int launch_encode_prefix(const EncodeArgs &a, void *stream)
{
    if (a.n_frames == 0)
        return hipSuccess;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t items = a.n_frames * static_cast<uint64_t>(a.words);
    hipLaunchKernelGGL(encode_info_kernel, dim3(static_cast<unsigned>((items + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(encode_prefix_kernel, dim3(a.words), dim3(1024), 0, s, a);
    return hipGetLastError();
}

int launch_encode_codewords(const EncodeArgs &a, void *stream, bool only_last)
{
    if (a.n_frames == 0)
        return hipSuccess;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = sizeof(uint64_t) * a.words;
    const bool all = !only_last && a.codeword;
    if (a.g_mask && a.words <= 4 && a.nc <= 256 * kEncCols)
    {
        const uint64_t first = all ? 0 : a.n_frames - 1, n_do = all ? a.n_frames : 1;
        const dim3 grid(static_cast<unsigned>((n_do + kEncFrames - 1) / kEncFrames));
        switch (a.words)
        {
        case 1: hipLaunchKernelGGL(encode_cw_dense_kernel<1>, grid, dim3(256), 0, s, a, first, n_do); break;
        case 2: hipLaunchKernelGGL(encode_cw_dense_kernel<2>, grid, dim3(256), 0, s, a, first, n_do); break;
        case 3: hipLaunchKernelGGL(encode_cw_dense_kernel<3>, grid, dim3(256), 0, s, a, first, n_do); break;
        default: hipLaunchKernelGGL(encode_cw_dense_kernel<4>, grid, dim3(256), 0, s, a, first, n_do); break;
        }
        return hipGetLastError();
    }
    if (all)
        hipLaunchKernelGGL(encode_cw_kernel, dim3(static_cast<unsigned>(a.n_frames)), dim3(256), lds, s, a, uint64_t(0));
    else
        hipLaunchKernelGGL(encode_cw_kernel, dim3(1), dim3(256), lds, s, a, a.n_frames - 1);
    return hipGetLastError();
}

int launch_encode(const EncodeArgs &a, void *stream)
{
    if (a.n_frames == 0)
        return hipSuccess;
    int rc = launch_encode_prefix(a, stream);
    if (rc != hipSuccess)
        return rc;
    return launch_encode_codewords(a, stream, a.codeword == nullptr); // (no codewords wanted: only the running one after the batch)
}

int launch_batch_counters(const uint32_t *iters, const uint32_t *bit_errors, uint64_t n, uint32_t max_iters, int early_term,
                          long long *counters, void *stream)
{
    hipLaunchKernelGGL(batch_counters_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), iters, bit_errors, n,
                       max_iters, early_term, counters);
    return hipGetLastError();
}

} // namespace ldpc_amd
