// kernels_layered_fixed_body.inc — a frame of fixed-point layered min-sum from the point where its quantized channel values
// stand in T[nc] (rank order) and the correction table in lut: the records cleared, the sweeps with the syndrome check after
// each, the outputs.  Included by decode_layered_fixed_kernel (kernels_layered_fixed.hip) and
// decode_layered_fixed_direct_kernel (kernels_layered_fixed_direct.hip): one text, compiled into each kernel as its own code
// (not through an inlined function, which changes the register allocation of the existing kernels; kernels_reg_body.inc).
// In scope: the template parameter WANT_LLR, the kernel arguments a, L, q, and P, nc, lane, frame, rec_slots, T, records,
// lut, cw, qmax, pmax as the kernels define them.
    for (uint32_t i = lane; i < rec_slots; i += 64)
        records[i] = 0; // every message 0: magnitudes 0, argmin 0, no sign bit
    __syncthreads();

    // the step's neighbour table one step AHEAD (kernels_layered.hip)
    const auto steps = uniform_table(reinterpret_cast<const uint32_t *>(L.steps));
    const auto rec_off = uniform_table(L.rec_off);
    const uint32_t *table = L.vn4 + lane;
    auto fetch = [&](uint32_t s, uint32_t (&pk)[4]) {
#pragma unroll
        for (int w = 0; w < 4; ++w)
            pk[w] = table[(s * 4 + w) * 64];
    };
    uint32_t I = 0;
    uint32_t nxt[4];
    fetch(0, nxt);
    while (I < a.iterations)
    {
        for (uint32_t s = 0; s < L.n_steps; ++s)
        {
            uint32_t cur[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
            fetch(s + 1 < L.n_steps ? s + 1 : 0, nxt); // (the sweep's last step fetches the first one's)
            const uint32_t cd = steps[2 * s + 1], ro = rec_off[s] / 20;
            const int count = cd & 0xFFFF, degree = cd >> 16;
            if (lane < count)
            {
                lds_u32 *rec = records + ro + lane;
                switch (degree) // wave-uniform
                {
                case 2: cn_layered_fixed<2>(T, rec, lut, cur, qmax, pmax); break;
                case 3: cn_layered_fixed<3>(T, rec, lut, cur, qmax, pmax); break;
                case 4: cn_layered_fixed<4>(T, rec, lut, cur, qmax, pmax); break;
                case 5: cn_layered_fixed<5>(T, rec, lut, cur, qmax, pmax); break;
                case 6: cn_layered_fixed<6>(T, rec, lut, cur, qmax, pmax); break;
                case 7: cn_layered_fixed<7>(T, rec, lut, cur, qmax, pmax); break;
                case 8: cn_layered_fixed<8>(T, rec, lut, cur, qmax, pmax); break;
                default: break;
                }
            }
            __builtin_amdgcn_wave_barrier(); // (LDS operations of a wave execute in order; this only stops the compiler)
        }
        // syndrome of the decisions after this sweep (decoder.cpp:66-72)
        if (a.early_term)
        {
            uint32_t bad = 0;
            for (uint32_t s = 0; s < L.n_steps; ++s)
            {
                uint32_t cur[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
                fetch(s + 1 < L.n_steps ? s + 1 : 0, nxt);
                const uint32_t cd = steps[2 * s + 1];
                const int count = cd & 0xFFFF, degree = cd >> 16;
                if (lane < count)
                {
                    switch (degree)
                    {
                    case 2: bad |= cn_parity_fixed<2>(T, cur); break;
                    case 3: bad |= cn_parity_fixed<3>(T, cur); break;
                    case 4: bad |= cn_parity_fixed<4>(T, cur); break;
                    case 5: bad |= cn_parity_fixed<5>(T, cur); break;
                    case 6: bad |= cn_parity_fixed<6>(T, cur); break;
                    case 7: bad |= cn_parity_fixed<7>(T, cur); break;
                    case 8: bad |= cn_parity_fixed<8>(T, cur); break;
                    default: break;
                    }
                }
            }
            if (__ballot(bad != 0) == 0)
                break;
        }
        ++I;
    }
    if (lane == 0 && a.iters)
        a.iters[frame] = I;
    const bool ran = a.iterations > 0;
    uint8_t *h = a.hard ? a.hard + frame * nc : nullptr;
    for (int r = lane; r < nc; r += 64)
    {
        const int x = T[r];
        if (h)
            h[P.rank_col[r]] = ran ? static_cast<uint8_t>(x <= 0) : 0; // mCO is still zero-initialised when no iteration ran
        if constexpr (WANT_LLR)
            a.llr_out[frame * nc + P.rank_col[r]] = ran ? static_cast<double>(x) * q.step : 0.0;
    }
    if (a.bit_errors)
    {
        int err = 0;
        for (int i = lane; i < P.n_bitpos; i += 64)
        {
            const int est = ran ? static_cast<int>(T[P.tx_rank[i]] <= 0) : 0;
            const int tx = cw ? static_cast<int>(cw[P.bit_pos[i]]) : 0;
            err += est != tx;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            err += __shfl_xor(err, o, 64);
        if (lane == 0)
            a.bit_errors[frame] = static_cast<uint32_t>(err);
    }
