// Body of k_generic_receive and k_generic_receive_burst (gfdm_generic.hip), included inside both kernel definitions: the burst kernel takes
// BurstIo as one more, last argument, and a body shared as text leaves the code of k_generic_receive exactly what it was.  Expects the
// template parameters GLOBAL, MX, the constant BURST, the kernel arguments pg, ic, est, eq_source, ntiles, mode, s_in_global, tab_off, ta,
// out, in, f_eq, and `bio` (BurstIo; read only where BURST).  No include guard: it is included once per kernel.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const DevicePlan p = stage_tables(pg, smem, tab_off);
    const auto mx = mx_of<MX>(p, ta, smem);
    float* red = reinterpret_cast<float*>(smem);
    cf* t0;
    if constexpr (GLOBAL) t0 = ta.gtiles + (int64_t)blockIdx.x * ta.tile_elems; else t0 = reinterpret_cast<cf*>(smem + RED_BYTES);
    const int M = p.M, K = p.K, L = p.L, N = p.N;
    const int TS = GLOBAL ? N : ta.tile_stride;
    cf* t1 = t0 + TS;
    cf* t2 = t1 + TS;                                              // only valid when 3 tiles were requested
    const int64_t blk = ta.blk0 + blockIdx.x;
    const cf* x = in + blk * (int64_t)(ic.io.in_stride ? ic.io.in_stride : N) + ic.io.in_offset;   // frame -> block
    const bool demap = ic.io.demap && mode != RX_FD;
    cf* o = out + blk * (demap ? ic.io.nout : N);
    const cf* eq = (eq_source == EQ_VECTOR) ? f_eq + blk * N : nullptr;
    cf* filt = t0 + (size_t)ntiles * TS + K;                      // EQ_PREAMBLE: smoothed channel estimate, behind the tiles
    int64_t cap_base = 0;
    int cap_rotate = 0;
    double cap_phi = 0.0;
    if constexpr (BURST) {
        // bursts from `count` on (the detector's spare slots) read nothing and yield zeros
        const int64_t cnt = bio.count ? *bio.count : blk + 1;
        if (blk >= cnt) {
            for (int idx = threadIdx.x; idx < (demap ? ic.io.nout : N); idx += GT) o[idx] = make_float2(0.f, 0.f);
            return;
        }
        cap_base = bio.off[blk] - bio.backoff;
        if (bio.rot) burst_phase_step(bio.rot[blk], cap_rotate, cap_phi);
    }
    if (eq_source == EQ_PREAMBLE) {                                // channel estimator in front, the tiles are its scratch
        cf* bins = t0 + (size_t)ntiles * TS;
        if constexpr (BURST)
            estimate_preamble_bins_from(est, [&](int i) { return burst_fetch(bio.cap, bio.fmt, bio.cap_len, cap_base, bio.pre + i, 1.f, cap_rotate, cap_phi); }, t0, t1, bins);
        else
        estimate_preamble_bins(est, f_eq + blk * (est.pre_stride ? est.pre_stride : 2 * K), t0, t1, bins);
        __syncthreads();
        for (int i = threadIdx.x; i < est.n_est; i += GT) filt[i] = est_filter_bin(bins, i, est);
        __syncthreads();
    }

    GFDM_GSTAMP(0);
    if constexpr (BURST) {
        for (int idx = threadIdx.x; idx < N; idx += GT) t1[idx] = burst_fetch(bio.cap, bio.fmt, bio.cap_len, cap_base, ic.io.in_offset + idx, 1.f, cap_rotate, cap_phi);
    } else {
        stream_in(t1, x, N);
    }
    __syncthreads();
    GFDM_GSTAMP(1);
    // A[q][m] = W_N^{q m} * sum_p x[K p + q] W_M^{p m}
    // (matrix-core form without a scratch of its own: the operands go to the free tile t0, the result replaces the samples in t1)
    cf* A0 = mx.in_place() ? t1 : t0;
    cf* A1 = mx.in_place() ? t0 : t1;
    paired_dft<false>(mx.at(t0, K), K, M, p.wM, [&](int q, int pp) { return t1[K * pp + q]; },       // outputs m and M - m from one pass (DftPair)
                      [&](int q, int m, const DftPair& acc) {
                          const int m2 = (m == 0) ? 0 : M - m;
                          A0[q * M + m] = cmul(acc.with_root(), p.wN[q * m]);
                          if (m2 != m) A0[q * M + m2] = cmul(acc.with_conj(), p.wN[q * m2]);
                      });
    __syncthreads();
    GFDM_GSTAMP(2);
    cf* X = col_fft<false>(A0, A1, p);                             // X[j][m] = FFT_N(x)[M j + m]       :304-305
    cf* U = (X == A0) ? A1 : A0;
    GFDM_GSTAMP(3);
    if (eq) {                                                      // one-tap equaliser                 :315-316
        stream_in(X, eq, N, [&](cf e, int idx) { return cdiv(X[idx], e); });
        __syncthreads();
    } else if (eq_source == EQ_PREAMBLE) {                         // same, the estimate interpolated on the fly
        for (int idx = threadIdx.x; idx < N; idx += GT) X[idx] = cdiv(X[idx], est_frame_bin<0>(filt, idx, est));
        __syncthreads();
    }
    // S[k][m] = sum_i taps[((i + L/2) % L) M + m] * X[((k + i + K - L/2) % K) M + m]                    :165-192
    cf* Sdst = (mode == RX_FD) ? o : U;
    if (L <= TAPS_IN_REGS) {
        for_columns(M, [&](int m, int k0, int ks) {
            cf tp[TAPS_IN_REGS];
#pragma unroll
            for (int i = 0; i < TAPS_IN_REGS; ++i) tp[i] = (i < L) ? p.taps[((i + L / 2) % L) * M + m] : make_float2(0.f, 0.f);
            int r0 = ((k0 - L / 2) % K + K) % K;                    // row (k + i - L/2) mod K, tap part (i + L/2) mod L
            const int rs = ks % K;
            for (int k = k0; k < K; k += ks) {
                cf acc = make_float2(0.f, 0.f);
                int row = r0;
#pragma unroll
                for (int i = 0; i < TAPS_IN_REGS; ++i) {
                    if (i < L) {
                        acc = cfma(tp[i], X[row * M + m], acc);
                        if (++row == K) row = 0;
                    }
                }
                Sdst[k * M + m] = acc;
                r0 += rs;
                if (r0 >= K) r0 -= K;
            }
        });
    } else {
        DivStep fx(threadIdx.x, GT, M);
        for (int idx = threadIdx.x; idx < N; idx += GT, fx.next()) {
            const int k = fx.q, m = fx.r;
            cf acc = make_float2(0.f, 0.f);
            int row = k - L / 2, part = L / 2;
            if (row < 0) row += K;
            for (int i = 0; i < L; ++i) {
                acc = cfma(p.taps[part * M + m], X[row * M + m], acc);
                if (++row == K) row = 0;
                if (++part == L) part = 0;
            }
            Sdst[idx] = acc;
        }
    }
    if (mode == RX_FD) return;
    __syncthreads();
    GFDM_GSTAMP(4);
    const float invM = 1.f / (float)M;
    if (mode == RX_DEMOD || ic.ic_iter <= 0) {
        if (!demap) {
            row_dft<true>(mx.at(X, K), o, U, K, M, M, 1, p.wM, invM);      // d = IFFT_M(S_k) / M                :211-225
            GFDM_GSTAMP(5);
        } else {
            cf* d = mx.in_place() ? U : X;                              // (X holds the operands then)
            row_dft<true>(mx.at(X, K), d, U, K, M, M, 1, p.wM, invM);
            __syncthreads();
            emit_demapped(o, d, ic.io, K, M);
        }
        return;
    }
    // One cancellation round of the reference is  d_new = IDFT_M(S - ic (.) DFT_M(nb)) / M  with nb = dec_{k-1} + dec_{k+1}
    // (receiver_kernel_cc.cc:274-299 + :211-225).  Both transforms are linear, so  d_new = d0 - g (*) nb  with d0 = IDFT_M(S) / M
    // and the M-tap circular kernel g = IDFT_M(ic) / M (p.icg): one table-driven pass per round instead of two, S is not needed
    // again (a rotation of S by the phase compensation is the same rotation of d0).
    cf* D = mx.in_place() ? t2 : X;                                // (in place: X takes the operands of every transform from here on)
    row_dft<true>(mx.at(X, K), D, U, K, M, M, 1, p.wM, invM);
    __syncthreads();
    if constexpr (MX) {
        // With the transforms on the matrix cores the rounds keep the reference's own form, S' = S - ic (.) DFT_M(nb), d = IDFT_M(S') / M: two constant-
        // matrix products per round instead of the O(M^2) convolution on the vector ALU.  S stays in its tile, S' goes to the third one (or the output block).
        cf* S = U;
        cf* V = mx.in_place() ? D : s_in_global ? o : t2;             // (in place: S' replaces the decisions once all of them are operands)
        const auto mxs = mx.at(X, K);
        for (int j = 0; j < ic.ic_iter; ++j) {
            if (ic.do_phase_compensation > 0 && j == 0) {
                const cf rot = phase_rotation(D, ic, red, M);
                for (int idx = threadIdx.x; idx < N; idx += GT) S[idx] = cmul(S[idx], rot);     // adv:63-70: the rotation of S persists
                __syncthreads();
            }
            {
                DivStep dx(threadIdx.x, GT, M);
                for (int idx = threadIdx.x; idx < N; idx += GT, dx.next())
                    D[idx] = ic.active[dx.q] ? decide(D[idx], ic) : make_float2(0.f, 0.f);
            }
            __syncthreads();
            cancel_rows(mxs, V, D, S, p);
            __syncthreads();
            const bool last = (j == ic.ic_iter - 1);
            row_dft<true>(mxs, (last && !demap) ? o : D, V, K, M, M, 1, p.wM, invM);
            __syncthreads();
            if (last && demap) emit_demapped(o, D, ic.io, K, M);
        }
        return;
    }
    cf* D0 = U;
    cf* V = t2;
    if (s_in_global) {                                            // third tile does not fit: d0 lives in the output block
        D0 = o;
        V = U;
    }
    for (int idx = threadIdx.x; idx < N; idx += GT) D0[idx] = D[idx];
    __syncthreads();
    for (int j = 0; j < ic.ic_iter; ++j) {                        // perform_ic_iterations            adv:56-76
        if (ic.do_phase_compensation > 0 && j == 0) {
            const cf rot = phase_rotation(D, ic, red, M);
            for (int idx = threadIdx.x; idx < N; idx += GT) D0[idx] = cmul(D0[idx], rot);   // rotating S rotates d0; persists  adv:63-70
            __syncthreads();
        }
        {
            DivStep dx(threadIdx.x, GT, M);
            for (int idx = threadIdx.x; idx < N; idx += GT, dx.next())   // map_symbols_to_constellation_points  adv:109-123
                D[idx] = ic.active[dx.q] ? decide(D[idx], ic) : make_float2(0.f, 0.f);
        }
        __syncthreads();
        {                                                         // nb = dec_{k-1} + dec_{k+1} (wraps mod K)  rx:279-284
            DivStep nx(threadIdx.x, GT, M);
            for (int idx = threadIdx.x; idx < N; idx += GT, nx.next()) {
                const int k = nx.q, pp = nx.r;
                V[idx] = cadd(D[(k == 0 ? K - 1 : k - 1) * M + pp], D[(k == K - 1 ? 0 : k + 1) * M + pp]);
            }
        }
        __syncthreads();
        const bool last = (j == ic.ic_iter - 1);
        cf* dst = (last && !demap) ? o : D;                        // the decisions are spent: the new symbols replace them
        DivStep cx(threadIdx.x, GT, M);
        for (int idx = threadIdx.x; idx < N; idx += GT, cx.next()) {
            const int pp = cx.r;
            const cf* nb = V + cx.q * M;
            cf acc = D0[idx];
            if (p.ic_real_sym) {                                   // g real and even: g_r (nb[p - r] + nb[p + r])
                const float g0 = p.icg[0].x;
                acc = make_float2(acc.x - g0 * nb[pp].x, acc.y - g0 * nb[pp].y);
                int lo = pp, hi = pp;
                const int H = (M - 1) / 2;
                for (int r = 1; r <= H; ++r) {
                    if (--lo < 0) lo = M - 1;
                    if (++hi == M) hi = 0;
                    const float g = p.icg[r].x;
                    acc = make_float2(acc.x - g * (nb[lo].x + nb[hi].x), acc.y - g * (nb[lo].y + nb[hi].y));
                }
                if ((M & 1) == 0) {                                // the middle tap of an even length
                    if (--lo < 0) lo = M - 1;
                    const float g = p.icg[M / 2].x;
                    acc = make_float2(acc.x - g * nb[lo].x, acc.y - g * nb[lo].y);
                }
            } else {
                int src = pp;                                     // (pp - r) mod M
                for (int r = 0; r < M; ++r) {
                    const cf g = p.icg[r], x = nb[src];
                    acc = make_float2(acc.x - g.x * x.x + g.y * x.y, acc.y - g.x * x.y - g.y * x.x);
                    if (--src < 0) src = M - 1;
                }
            }
            dst[idx] = acc;
        }
        __syncthreads();
        if (last && demap) emit_demapped(o, D, ic.io, K, M);
    }
