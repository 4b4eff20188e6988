// kernels_reg_body.inc — the body of the messages-form register-resident kernels (kernels_reg.hip), included by
// decode_reg_kernel and decode_reg_msc_kernel: one text, compiled into each kernel as its own code (not through an inlined
// function, which changes the register allocation of the existing kernels).  In scope: the template parameters MINSUM,
// WANT_LLR, NT, KC, MAXD, RATIO, SH6, the constant CORR (the corrected min-sum rule, device_cn.hpp) and the kernel
// arguments a, R.
    static_assert(!(RATIO && MINSUM), "the ratio form is a sum-product form");
    static_assert(RATIO || !SH6, "shared reciprocals belong to the ratio form");
    constexpr int kRegWaves = NT / 64;
    extern __shared__ double mb[]; // mailbox: mb_doubles doubles, then mb_doubles hard-bit bytes
    __shared__ int misc[4];
    uint8_t *hbm = reinterpret_cast<uint8_t *>(mb + R.mb_doubles);
    const DevPlan &P = a.plan;
    const int nc = P.nc;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    __builtin_amdgcn_s_setprio(3); // ahead of the noise generator's waves in the SIMD's instruction arbitration (kernels.hip)
    uint64_t frame = blockIdx.x;
    if (a.redo_count_in) // second pass: only the frames the ratio form handed back
    {
        if (blockIdx.x >= *uniform_table(a.redo_count_in))
            return;
        frame = uniform_table(a.redo_list_in)[blockIdx.x];
    }
    double *llr = a.ws_llr + frame * nc;
    uint8_t *hard = a.ws_hb + frame * nc;
    const uint8_t *cw = a.codeword ? a.codeword + frame * nc : nullptr;

    if (tid == 0)
        misc[0] = 0;
    channel_init<NT, kNoiseAny>(a, frame, llr, tid);
    __syncthreads();
    if (a.llr_in_dump)
    {
        double *o = a.llr_in_dump + frame * nc;
        for (int r = tid; r < nc; r += NT)
            o[P.rank_col[r]] = llr[r];
    }
    uint32_t escaped = 0; // RATIO: running maximum of dm_ratio_key over the frame's checked values (detmath.h)
    if constexpr (RATIO)
    {
        // input LLRs become lambda = e^-L in place (isolated variable nodes keep their LLR)
        for (int r = tid; r < nc; r += NT)
            if (P.rank_slot0[r] != kNoSlot)
            {
                const double L = llr[r];
                if (dm_ratio_llr_refused(L))
                    escaped = ~0u;
                llr[r] = dm_exp_clamped(0.0 - L);
            }
        __syncthreads();
    }

    double m[KC][MAXD];
    int deg[KC];
    bool have[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k)
    {
        deg[k] = R.cn_deg[k * kRegWaves + wave];
        have[k] = lane < static_cast<int>(R.cn_cnt[k * kRegWaves + wave]);
#pragma unroll
        for (int j = 0; j < MAXD; ++j)
            m[k][j] = 0.0;
    }
    const uint32_t *my_edge = R.cn_edge + tid;

    // ---- v2c initialisation (decoder.cpp:16-19): every edge starts with its VN's input LLR ----
    for (int r = 0; r < R.rounds; ++r)
    {
        for (uint32_t b = uniform_table(R.round_first)[r] + wave; b < uniform_table(R.round_first)[r + 1]; b += kRegWaves)
        {
            const RegVnBlock vb = load_block3(R.vn_blocks, b);
            if (lane < vb.count)
            {
                const double L = llr[vb.first + lane];
                const double v0 = RATIO ? dm_ratio_div(1.0, L) : L; // RATIO: L is lambda(L_ch), the first v2c is rho(L_ch)
                for (int p = 0; p < vb.degree; ++p)
                    mb[vb.mb_off + p * vb.count + lane] = v0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KC; ++k)
#pragma unroll
            for (int j = 0; j < MAXD; ++j)
            {
                const uint32_t e = my_edge[(k * MAXD + j) * NT];
                if (e != kRegNoEdge && (e >> 28) == static_cast<uint32_t>(r))
                    m[k][j] = mb[e & 0x0FFFFFFFu];
            }
        __syncthreads();
    }

    double *out_llr = WANT_LLR ? a.llr_out + frame * nc : nullptr;
    uint32_t I = 0;
    while (I < a.iterations)
    {
        // ---- CN pass (decoder.cpp:25-45), entirely in registers ----
        // (a fold expression, not a loop: every m[k] must be a compile-time register row)
        [&]<int... Ks>(std::integer_sequence<int, Ks...>) {
            ((have[Ks] ? cn_regs<MINSUM, RATIO, MAXD, SH6, CORR>(m[Ks], deg[Ks], &escaped, ms_corr<CORR>(a)) : void()), ...);
        }(std::make_integer_sequence<int, KC>{});

        int par[KC];
#pragma unroll
        for (int k = 0; k < KC; ++k)
            par[k] = 0;
        for (int r = 0; r < R.rounds; ++r)
        {
            // c2v -> mailbox
#pragma unroll
            for (int k = 0; k < KC; ++k)
#pragma unroll
                for (int j = 0; j < MAXD; ++j)
                {
                    const uint32_t e = my_edge[(k * MAXD + j) * NT];
                    if (e != kRegNoEdge && (e >> 28) == static_cast<uint32_t>(r))
                        mb[e & 0x0FFFFFFFu] = m[k][j];
                }
            __syncthreads();
            // ---- VN pass, APP and hard decision (decoder.cpp:48-64) on this round's VN blocks ----
            for (uint32_t b = uniform_table(R.round_first)[r] + wave; b < uniform_table(R.round_first)[r + 1]; b += kRegWaves)
            {
                const RegVnBlock vb = load_block3(R.vn_blocks, b);
                if (lane < vb.count)
                {
                    const int rank = vb.first + lane;
                    double *col = mb + vb.mb_off + lane;
                    uint8_t *hcol = hbm + vb.mb_off + lane;
                    if constexpr (RATIO)
                        if (vb.degree > 0)
                        {
                            if (vb.degree == 1)
                            {
                                // a leaf: its v2c is the channel ratio itself, the decision lambda(c2v) >= rho_ch
                                // (kernels.hip, vn_leaf_ratio)
                                const double c = col[0], rho = dm_ratio_div(1.0, llr[rank]);
                                const uint8_t lbit = c >= rho;
                                col[0] = rho;
                                hcol[0] = lbit;
                                hard[rank] = lbit;
                                if constexpr (WANT_LLR)
                                    out_llr[P.rank_col[rank]] = 0.0 - dm_log(dm_ratio_div(c, rho));
                                continue;
                            }
                            // lambda(total) = lambda(L_ch) * prod lambda(c2v_p), in column file order
                            double prod = llr[rank];
                            if (vb.degree <= 3)
                                for (int p = 0; p < vb.degree; ++p)
                                    prod *= col[p * vb.count];
                            else
                                for (int p = 0; p < vb.degree; ++p)
                                {
                                    prod *= col[p * vb.count];
                                    if (p % 3 == 2)
                                        DM_RATIO_TRACK(escaped, prod);
                                }
                            const uint8_t bit = prod >= 1.0; // total LLR <= 0
                            const double tot = dm_ratio_div(1.0, prod);   // rho(total)
                            for (int p = 0; p < vb.degree; ++p)
                            {
                                const double o = tot * col[p * vb.count]; // rho(total - c2v_p)
                                DM_RATIO_TRACK(escaped, o);
                                col[p * vb.count] = o;
                                hcol[p * vb.count] = bit;
                            }
                            hard[rank] = bit;
                            if constexpr (WANT_LLR)
                                out_llr[P.rank_col[rank]] = 0.0 - dm_log(prod);
                            continue;
                        }
                    double out = llr[rank];
                    for (int p = 0; p < vb.degree; ++p) // sequential sum in column file order
                        out += col[p * vb.count];
                    const uint8_t bit = out <= 0;
                    for (int p = 0; p < vb.degree; ++p)
                    {
                        col[p * vb.count] = out - col[p * vb.count];
                        hcol[p * vb.count] = bit;
                    }
                    hard[rank] = bit;
                    if constexpr (WANT_LLR)
                        out_llr[P.rank_col[rank]] = out;
                }
            }
            __syncthreads();
            // v2c (and the hard decision of the edge's VN) <- mailbox
#pragma unroll
            for (int k = 0; k < KC; ++k)
#pragma unroll
                for (int j = 0; j < MAXD; ++j)
                {
                    const uint32_t e = my_edge[(k * MAXD + j) * NT];
                    if (e != kRegNoEdge && (e >> 28) == static_cast<uint32_t>(r))
                    {
                        m[k][j] = mb[e & 0x0FFFFFFFu];
                        par[k] ^= hbm[e & 0x0FFFFFFFu];
                    }
                }
            __syncthreads();
        }
        // ---- syndrome early termination (decoder.cpp:66-72, decoder.h:47-64) ----
        if constexpr (RATIO)
            if (__syncthreads_or(DM_RATIO_ESCAPED(escaped))) // checked before the syndrome: an escaped frame's hard decisions mean nothing
            {
                if (tid == 0)
                    a.redo_list[atomicAdd(a.redo_count, 1u)] = static_cast<uint32_t>(frame);
                return;
            }
        if (a.early_term)
        {
            int bad = 0;
#pragma unroll
            for (int k = 0; k < KC; ++k)
                bad |= have[k] ? par[k] : 0;
            if (!__syncthreads_or(bad))
                break;
        }
        ++I;
    }
    __syncthreads();

    // ---- outputs ----
    if (tid == 0 && a.iters)
        a.iters[frame] = I;
    const bool ran = a.iterations > 0;
    if (a.hard)
    {
        uint8_t *h = a.hard + frame * nc;
        for (int r = tid; r < nc; r += NT)
            h[P.rank_col[r]] = ran ? hard[r] : 0;
    }
    if constexpr (WANT_LLR)
    {
        if (!ran)
            for (int r = tid; r < nc; r += NT)
                out_llr[P.rank_col[r]] = 0.0;
    }
    if (a.bit_errors)
    {
        int err = 0;
        for (int i = tid; i < P.n_bitpos; i += NT)
        {
            int est = ran ? hard[P.tx_rank[i]] : 0;
            int tx = cw ? static_cast<int>(cw[P.bit_pos[i]]) : 0;
            err += est != tx;
        }
        err = wave_sum(err);
        if (lane == 0 && err)
            atomicAdd(&misc[0], err);
        __syncthreads();
        if (tid == 0)
            a.bit_errors[frame] = static_cast<uint32_t>(misc[0]);
    }
