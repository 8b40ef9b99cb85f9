// Body of k_row_receive and k_row_receive_burst (gfdm_rowlane_impl.h), included inside both kernel definitions: the two kernels differ in their
// argument list (the burst kernel takes BurstIo as one more, last argument), and a body shared as text leaves the code of k_row_receive exactly
// what it was -- shared through an inlined function its kernels came out with other register counts.  Expects the template parameters
// K, M, L, MODE, EQT (EqSource; EQ_BURST = the gather-load form), ICK, the kernel arguments p, ic, est, twT, out, in, f_eq, nblocks, and `bio`
// (BurstIo; read only where EQT == EQ_BURST).  No include guard: it is included once per kernel.
    using S = RowShape<K>;
    constexpr bool BURST = (EQT == EQ_BURST);
    constexpr int EQ = BURST ? (int)EQ_PREAMBLE : EQT;
    constexpr int MS = (EQ == EQ_PREAMBLE) ? M + 2 : M;   // tile row stride: with EQ_PREAMBLE two extra columns carry the preamble halves
    using T = RowTile<K, MS>;
    constexpr int N = K * M;
    constexpr bool ICSYM = (ICK == ICK_REALSYM);
    constexpr bool ICMX = (MODE == RX_IC && ICK == ICK_MFMA);   // cancellation rounds on the matrix cores (IcMfma)
    static_assert(!ICMX || rowgeom::ic_mfma(K, M), "IcMfma: K a power of two >= 16, 4 <= M <= 16");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int g = threadIdx.x / K, q = threadIdx.x - g * K;            // q doubles as row index k in phase D
    const int64_t blk = (int64_t)blockIdx.x * S::BPW + g;
    const bool valid = blk < nblocks;
    const int64_t base = (valid ? blk : 0) * N;
    const int64_t in_base = (valid ? blk : 0) * (int64_t)(ic.io.in_stride ? ic.io.in_stride : N) + ic.io.in_offset;   // frame -> block
    cf* X = reinterpret_cast<cf*>(smem) + g * T::TS;                   // the block's single LDS tile, [row][M]

    GFDM_STAMP(0);
    // EQ_BURST: the per-burst scalars the sample addresses depend on -- count, offset, r_b -- are requested first of all; bursts from
    // `count` on (the detector's spare slots) read nothing and store zeros
    bool live = valid;
    int64_t cap_base = 0, cap_len = 0;
    int cap_rotate = 0;
    double cap_phi = 0.0;
    (void)live; (void)cap_base; (void)cap_len; (void)cap_rotate; (void)cap_phi;
    if constexpr (BURST) {
        if (bio.count) {
            const int64_t cnt = *bio.count;
            live = blk < cnt;
        }
        live = live && valid;
        if (live) {
            cap_base = bio.off[blk] - bio.backoff;
            cap_len = bio.cap_len;                         // (0 for the others: every sample of theirs is out of bounds)
            if (bio.rot) burst_phase_step(bio.rot[blk], cap_rotate, cap_phi);
        }
    }
    // ---- phase A: timeslot DFT of row q, twiddle W_N^{q m}
    cf v[M];
    // K = 64 with PLAN_WIDE_IO (launch-uniform; packed blocks, in_base == base): 16-byte sample accesses, gfdm_rowlane_impl.h
    constexpr bool WIDE_IN = (K == 64 && !BURST && kWideRxIn), WIDE_OUT = (K == 64 && !BURST && !ICMX && kWideRxOut);
    const bool wide = (K == 64) && (p.taps_real & PLAN_WIDE_IO) != 0;
    (void)wide;
    if constexpr (!BURST) {
        bool loaded = false;
        if constexpr (WIDE_IN) {
            if (wide) { wide_load_rows<M>(v, in + in_base, q); loaded = true; }
        }
        if (!loaded) static_for<0, M>([&](auto pi) { constexpr int pp = decltype(pi)::value; v[pp] = ld_stream(in + in_base + K * pp + q); });
    }
    FftTwiddles<K> twd;
    load_fft_twiddles<K, rowgeom::packed_roots(K, M)>(twd, q, p.wK);
    // Everything else the later phases read from global memory is requested here as well: behind an ordering point a load can
    // only be issued where it is needed, and its round trip (scalar cache for the uniform tables, L1 / L2 for the per-lane
    // ones) lands on the wave's critical path.  Filter and IC taps are uniform (SGPRs) and only preloaded while they fit.
    constexpr bool PRE_TAPS = (L * M <= 24);
    cf tapv[PRE_TAPS ? L * M : 1], icgv[(PRE_TAPS && MODE == RX_IC) ? M : 1];
    if constexpr (PRE_TAPS) {
        static_for<0, L * M>([&](auto ii) { constexpr int i = decltype(ii)::value; tapv[i] = p.taps[i]; });
        if constexpr (MODE == RX_IC) static_for<0, M>([&](auto ii) { constexpr int i = decltype(ii)::value; icgv[i] = p.icg[i]; });
    }
    auto tap = [&](auto ii) { constexpr int i = decltype(ii)::value; if constexpr (PRE_TAPS) return tapv[i]; else return p.taps[i]; };
    const bool treal = (K == 64) ? (p.taps_real & PLAN_TAPS_REAL) != 0 : p.taps_real != 0;
    auto icg = [&](auto ii) { constexpr int i = decltype(ii)::value; if constexpr (PRE_TAPS && MODE == RX_IC) return icgv[i]; else return p.icg[i]; };
    const int wgt = (MODE == RX_IC && !ICMX) ? ic.active[q] : 0;      // multiplicity of subcarrier k in subcarrier_map (0 = inactive)
    typename IcMfma<ICMX ? K : 16, ICMX ? M : 4>::Pre icpre;
    if constexpr (ICMX) IcMfma<K, M>::preload(icpre, p, ic);
    const int rank_q = (MODE != RX_FD && ic.io.demap) ? ic.io.rank[q] : -1;
    // ... and the scalar settings the later phases branch on (kernel arguments, i.e. scalar loads at the point of use otherwise)
    const int io_demap = ic.io.demap, io_nout = ic.io.nout, io_per_timeslot = ic.io.per_timeslot, io_A = ic.io.A;
    const int ic_iter = ic.ic_iter, ic_decision = ic.decision, ic_pc = ic.do_phase_compensation;
    GFDM_STAMP(1);
    // EQ_PREAMBLE: the received preamble's two halves ride through the subcarrier FFT as columns M and M + 1 of the tile
    cf pre0, pre1, inv0, inv1;
    if constexpr (BURST) {
        const int n0 = ic.io.in_offset + q, np = bio.pre + q;
        static_for<0, M>([&](auto pi) { constexpr int pp = decltype(pi)::value; v[pp] = burst_fetch(bio.cap, bio.fmt, cap_len, cap_base, n0 + K * pp, 1.f, cap_rotate, cap_phi); });
        pre0 = burst_fetch(bio.cap, bio.fmt, cap_len, cap_base, np, 1.f, cap_rotate, cap_phi);
        pre1 = burst_fetch(bio.cap, bio.fmt, cap_len, cap_base, np + K, 1.f, cap_rotate, cap_phi);
        inv0 = est.inv0[q];
        inv1 = est.inv1[q];
    } else if constexpr (EQ == EQ_PREAMBLE) {
        const cf* pre = f_eq + (valid ? blk : 0) * (int64_t)(est.pre_stride ? est.pre_stride : 2 * K);
        pre0 = ld_stream(pre + q);
        pre1 = ld_stream(pre + K + q);
        inv0 = est.inv0[q];
        inv1 = est.inv1[q];
    }
    cf tw[M];
    load_row_twiddles<K, M>(tw, twT, q);
    dft_inplace<M, false>(v);
    constexpr bool REGPASS = (K == 64) && kRegFirstPass;
    if constexpr (REGPASS) {
        cf rowv[MS];
        rowv[0] = v[0];
        static_for<1, M>([&](auto mi) { constexpr int m = decltype(mi)::value; rowv[m] = cmul(v[m], tw[m]); });
        if constexpr (EQ == EQ_PREAMBLE) { rowv[M] = pre0; rowv[M + 1] = pre1; }
        wave_fft_first_pass<MS, false>(X, q, twd, rowv);
    } else {
        cf* xa = X + FftLayout<K>::slot(q) * MS;                   // row q goes to its FFT slot
        xa[0] = v[0];
        static_for<1, M>([&](auto mi) { constexpr int m = decltype(mi)::value; xa[m] = cmul(v[m], tw[m]); });
        if constexpr (EQ == EQ_PREAMBLE) { xa[M] = pre0; xa[M + 1] = pre1; }
        block_sync<K>();
    }
    // The equaliser vector is needed only after the subcarrier FFT: request it now, behind every wave's sample loads
    // (HBM serves requests roughly in issue order, so the samples of all waves arrive first and the transforms start
    // earlier; f_eq streams in while phases A/B run).
    constexpr bool ROWREG = (K == 64 && L == 2 && EQ == EQ_PREAMBLE && !(ICMX && kIcRegTranspose));   // equalised row stays in registers between phases C and D
    cf xrow[ROWREG ? M : 1];
    cf heq[EQ == EQ_VECTOR ? M : 1];
    if constexpr (EQ == EQ_VECTOR) {
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, M>([&](auto ii) { constexpr int i = decltype(ii)::value; heq[i] = ld_stream(f_eq + base + q + K * i); });
    }

    // ---- phase B: subcarrier FFT, in place
    lds_subcarrier_fft<K, MS, false, REGPASS ? 1 : 0>(X, q, twd);

    GFDM_STAMP(2);
    // ---- phase C: X[f] / f_eq[f] in linear order (a conj(b) / |b|^2, reciprocal by v_rcp_f32)              rx:315-316
    if constexpr (EQ == EQ_VECTOR) {
        static_for<0, M>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            const cf a = X[q + K * i], b = heq[i];
            const float inv = __builtin_amdgcn_rcpf(b.x * b.x + b.y * b.y);
            X[q + K * i] = mk((a.x * b.x + a.y * b.y) * inv, (a.y * b.x - a.x * b.y) * inv);
        });
        block_sync<K>();
    } else if constexpr (EQ == EQ_PREAMBLE) {
        // lane q holds estimate bin q (est:118-145): scatter it to its place in the fftshift-ordered, edge-replicated array the
        // smoothing filter runs over                                                                       est:147-175
        cf* inter = reinterpret_cast<cf*>(smem + row_lds_bytes<K, MS>()) + g * EstTile<K>::FS;
        cf* F = X + M;                                     // smoothed bin i -> column M of row i (dead once its lane has read it)
        const cf eq = cfma(X[q * MS + M], inv0, cmul(X[q * MS + M + 1], inv1));
        const int pos = est_active_pos(q, est), n_est = est.n_est;
        if (pos >= 0) {
            inter[4 + pos] = eq;
            if (pos == 0) { inter[0] = eq; inter[1] = eq; inter[2] = eq; inter[3] = eq; }
            if (pos == n_est - 1) { inter[n_est + 4] = eq; inter[n_est + 5] = eq; inter[n_est + 6] = eq; inter[n_est + 7] = eq; }
        }
        block_sync<K>();
        if (est.dc_free) {                                                         // DC bin: mean of its neighbours
            if (q == 0) {
                const cf lo = inter[4 + est.A / 2 - 1], hi = inter[4 + est.A / 2 + 1];
                inter[4 + est.A / 2] = mk(0.5f * (lo.x + hi.x), 0.5f * (lo.y + hi.y));
            }
            block_sync<K>();
        }
        if (q < n_est) {                                                           // 9-tap Gaussian         est:176-187
            cf acc = mk(0.f, 0.f);
            static_for<0, 9>([&](auto ti) {
                constexpr int t = decltype(ti)::value;
                const cf x = inter[q + t];
                acc.x += x.x * est.gauss[t];
                acc.y += x.y * est.gauss[t];
            });
            F[q * MS] = acc;
        }
        block_sync<K>();
        // row q = bins M q .. M q + M - 1 lies inside one interpolation segment of the smoothed estimate   est:238-273
        cf lo, hi;
        est_row_segment(F, MS, q, est, lo, hi);
        const cf dlt = mk(hi.x - lo.x, hi.y - lo.y);
        constexpr float step = 1.0f / (float)M;
        static_for<0, M>([&](auto mi) {
            constexpr int m = decltype(mi)::value;
            const float t = (float)m * step;
            const cf a = X[q * MS + m], b = mk(lo.x + dlt.x * t, lo.y + dlt.y * t);
            const float inv = __builtin_amdgcn_rcpf(b.x * b.x + b.y * b.y);
            const cf e = mk((a.x * b.x + a.y * b.y) * inv, (a.y * b.x - a.x * b.y) * inv);
            if constexpr (ROWREG) xrow[m] = e; else X[q * MS + m] = e;      // ROWREG: phase D takes the row from registers
        });
        if constexpr (!ROWREG) block_sync<K>();
    }

    // ---- phase D: S[k][m] = sum_i taps[((i + L/2) % L) M + m] X[(k + i - L/2) mod K][m]                      rx:165-192
    // (the matrix-core rounds want the rows of a block dealt to the lanes in IcMfma's order: kq instead of q from here to the rounds)
    int kq = q;
    if constexpr (ICMX) kq = IcMfma<K, M>::row_of(q);
    cf s[M];
    static_for<0, M>([&](auto mi) { constexpr int m = decltype(mi)::value; s[m] = mk(0.f, 0.f); });
    auto filter = [&](auto real_tag) {                     // one copy per kind of taps, chosen by a uniform branch
        constexpr bool TREAL = decltype(real_tag)::value;
        if constexpr (K == 64 && L == 2 && !(ICMX && kIcRegTranspose)) {
            // the block IS the wavefront and the only foreign row is k - 1 = lane k - 1: a DPP wave rotate of the own row replaces the
            // second LDS row read
            const cf* rb = X + q * MS;
            static_for<0, M>([&](auto mi) {
                constexpr int m = decltype(mi)::value;
                cf own;
                if constexpr (ROWREG) own = xrow[m]; else own = rb[m];
                const cf below = mk(dpp_wave_ror1(own.x), dpp_wave_ror1(own.y));
                s[m] = tap_fma<TREAL>(tap(std::integral_constant<int, M + m>{}), below, s[m]);       // i = 0: row k - 1
                s[m] = tap_fma<TREAL>(tap(std::integral_constant<int, m>{}), own, s[m]);             // i = 1: row k
            });
        } else {
            static_for<0, L>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                const cf* rb = X + wrap_k<K>(kq + i - L / 2 + K) * MS;
                static_for<0, M>([&](auto mi) {
                    constexpr int m = decltype(mi)::value;
                    s[m] = tap_fma<TREAL>(tap(std::integral_constant<int, ((i + L / 2) % L) * M + m>{}), rb[m], s[m]);
                });
            });
        }
    };
    if (treal) filter(std::true_type{}); else filter(std::false_type{});
    constexpr float invM = 1.0f / (float)M;
    cf d[M];
    if constexpr (MODE != RX_FD) {
        // from here on S only feeds inverse DFTs that are scaled by 1/M: fold the scale into S (and into the IC taps)
        static_for<0, M>([&](auto mi) { constexpr int m = decltype(mi)::value; s[m] = scale(s[m], invM); d[m] = s[m]; });
        dft_inplace<M, true>(d);                                                                         // rx:211-225
    }
    block_sync<K>();                                      // every lane has read its neighbour rows: the tile is free
    GFDM_STAMP(3);

    if constexpr (ICMX) {
        constexpr size_t edge_off = (EQ == EQ_PREAMBLE) ? row_lds_bytes<K, MS>() + EstTile<K>::bytes : row_lds_bytes<K, M>();
        IcMfma<K, M>::template rounds<T::TS>(smem, smem + edge_off + rowgeom::ic_mfma_pad_bytes(K), X, q, d, icpre, ic_iter);
    } else if constexpr (MODE == RX_IC) {
        // One cancellation round of the reference is  d_new = IDFT_M(S - ic (.) DFT_M(nb)) / M  with nb = dec_{k-1} + dec_{k+1}.
        // Both transforms are linear, so  d_new = d0 - g (*) nb  with d0 = IDFT_M(S)/M (already in d) and the M-tap circular
        // convolution kernel g = IDFT_M(ic)/M (host table p.icg).  For the usual real, even prototype filters ic is real and
        // symmetric, hence g is too (ICSYM): M(M+1)/2 packed multiply-adds per row and round instead of two M-point DFTs.
        float* red = reinterpret_cast<float*>(reinterpret_cast<cf*>(smem) + S::BPW * T::TS);
        cf d0[M];
        static_for<0, M>([&](auto mi) { constexpr int m = decltype(mi)::value; d0[m] = d[m]; });
        for (int it = 0; it < ic_iter; ++it) {                                                           // adv:56-76
            const bool pc = (ic_pc > 0) && (it == 0);
            float acc = 0.f;
            cf dec[M];
            if (ic_decision == 1 && !pc) {
                // QPSK hot path (constellation_qpsk::decision_maker: sign tests, zero -> negative point); the per-lane
                // amplitudes are 0 on inactive subcarriers, so one compare + one select per component           adv:109-123
                const float sp = (wgt > 0) ? 0.70710678118654752f : 0.f, sn = -sp;
                static_for<0, M>([&](auto mi) {
                    constexpr int m = decltype(mi)::value;
                    dec[m] = mk(d[m].x > 0.f ? sp : sn, d[m].y > 0.f ? sp : sn);
                });
            } else {
                static_for<0, M>([&](auto mi) {                                                          // adv:109-123
                    constexpr int m = decltype(mi)::value;
                    dec[m] = (wgt > 0) ? decide_point(d[m], ic) : mk(0.f, 0.f);
                    if (pc && wgt > 0) acc += (float)wgt * (atan2f(dec[m].y, dec[m].x) - atan2f(d[m].y, d[m].x));
                });
            }
            if (pc) {                                                                                    // adv:59-71, 78-91
                if constexpr (S::LDS_REDUCE) {
                    // the block's lanes are not aligned to wavefronts: sum through the (free) tile
                    float* part = reinterpret_cast<float*>(X);
                    part[q] = acc;
                    block_sync<K>();
                    acc = 0.f;
                    for (int i = 0; i < K; ++i) acc += part[i];
                    block_sync<K>();
                } else {
                    for (int off = 1; off < 64 && off < K; off <<= 1) acc += __shfl_xor(acc, off, 64);
                    if constexpr (K > 64) {
                        if ((q & 63) == 0) red[q >> 6] = acc;
                        block_sync<K>();
                        acc = 0.f;
                        static_for<0, K / 64>([&](auto wi) { acc += red[decltype(wi)::value]; });
                    }
                }
                const float phi = acc / (float)(ic.n_active * M);
                float sn, cs;
                sincosf(phi, &sn, &cs);
                const cf rot = mk(cs, sn);
                static_for<0, M>([&](auto mi) { constexpr int m = decltype(mi)::value; d0[m] = cmul(d0[m], rot); });   // rotating S rotates d0
            }
            // neighbours k-1 and k+1 (wrap mod K)                                                           rx:274-299
            cf nb[M];
            if constexpr (K == 64) {
                // the block IS the wavefront: subcarrier k +- 1 is lane +- 1 with wrap-around, i.e. a DPP wave rotate --
                // no LDS traffic and no ordering point in the whole cancellation round
                static_for<0, M>([&](auto mi) {
                    constexpr int m = decltype(mi)::value;
                    nb[m] = mk(dpp_wave_ror1(dec[m].x) + dpp_wave_rol1(dec[m].x), dpp_wave_ror1(dec[m].y) + dpp_wave_rol1(dec[m].y));
                });
            } else {
                static_for<0, M>([&](auto mi) { constexpr int m = decltype(mi)::value; X[q * M + m] = dec[m]; });
                block_sync<K>();
                const cf* below = X + wrap_k<K>(q - 1 + K) * M;
                const cf* above = X + wrap_k<K>(q + 1) * M;
                static_for<0, M>([&](auto mi) { constexpr int m = decltype(mi)::value; nb[m] = below[m] + above[m]; });
            }
            if constexpr (ICSYM) {
                // real symmetric kernel: both components of a term share the real factor -> one packed v_pk_fma_f32 per term
                // (and one v_pk_add_f32 per symmetric pair)
                typedef float v2f __attribute__((ext_vector_type(2)));
                constexpr int H = (M - 1) / 2;
                v2f nv[M];
                static_for<0, M>([&](auto mi) { constexpr int m = decltype(mi)::value; nv[m] = v2f{ nb[m].x, nb[m].y }; });
                static_for<0, M>([&](auto pi) {
                    constexpr int pp = decltype(pi)::value;
                    const float g0 = -icg(std::integral_constant<int, 0>{}).x;
                    v2f acc = __builtin_elementwise_fma(nv[pp], v2f{ g0, g0 }, v2f{ d0[pp].x, d0[pp].y });
                    static_for<1, H + 1>([&](auto ri) {
                        constexpr int r = decltype(ri)::value;
                        const float gr = -icg(std::integral_constant<int, r>{}).x;
                        acc = __builtin_elementwise_fma(nv[(pp - r + M) % M] + nv[(pp + r) % M], v2f{ gr, gr }, acc);
                    });
                    if constexpr (M % 2 == 0) {
                        const float gm = -icg(std::integral_constant<int, M / 2>{}).x;
                        acc = __builtin_elementwise_fma(nv[(pp + M / 2) % M], v2f{ gm, gm }, acc);
                    }
                    d[pp] = mk(acc.x, acc.y);
                });
            } else {
                static_for<0, M>([&](auto pi) {
                    constexpr int pp = decltype(pi)::value;
                    cf acc = d0[pp];
                    static_for<0, M>([&](auto ri) {
                        constexpr int r = decltype(ri)::value;
                        const cf g = icg(std::integral_constant<int, r>{}), x = nb[(pp - r + M) % M];
                        acc = mk(fmaf(-g.x, x.x, fmaf(g.y, x.y, acc.x)), fmaf(-g.x, x.y, fmaf(-g.y, x.x, acc.y)));
                    });
                    d[pp] = acc;
                });
            }
            if constexpr (K != 64) block_sync<K>();       // all neighbour reads done before the tile is rewritten
        }
    }

    GFDM_STAMP(4);
    if (MODE != RX_FD && io_demap) {
        // resource demapper fused into the store: only active subcarriers, in mapper order; for per-timeslot order the lanes of
        // one timeslot write consecutive output symbols, so no LDS staging is needed                     mapper:91-106,136-163
        const int a = rank_q;
        if constexpr (ICMX) static_for<0, M>([&](auto mi) { constexpr int m = decltype(mi)::value; d[m] = X[IcMfma<ICMX ? K : 16, ICMX ? M : 4>::pa(q, m)]; });
        if (valid && a >= 0) {
            cf* o = out + blk * (int64_t)io_nout;
            static_for<0, M>([&](auto mi) {
                constexpr int m = decltype(mi)::value;
                const int idx = io_per_timeslot ? (m * io_A + a) : (a * M + m);
                if constexpr (BURST) { if (idx < io_nout) st_stream(o, idx, live ? d[m] : mk(0.f, 0.f)); }
                else if (idx < io_nout) st_stream(o, idx, d[m]);
            });
        }
    } else {
        // ---- output: row -> tile, linear read, coalesced store
        if constexpr (!ICMX) {                              // (IcMfma leaves its result in the tile)
            static_for<0, M>([&](auto mi) { constexpr int m = decltype(mi)::value; X[q * M + m] = (MODE == RX_FD) ? s[m] : d[m]; });
            block_sync<K>();
        }
        if constexpr (BURST) {
            if (valid) static_for<0, M>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                cf r;
                if constexpr (ICMX) r = X[IcMfma<ICMX ? K : 16, ICMX ? M : 4>::pa_linear(q + K * i)]; else r = X[q + K * i];
                st_stream(out, base + q + K * i, live ? r : mk(0.f, 0.f));
            });
        } else if (valid) {
            if constexpr (ICMX) static_for<0, M>([&](auto ii) { constexpr int i = decltype(ii)::value; st_stream(out, base + q + K * i, X[IcMfma<ICMX ? K : 16, ICMX ? M : 4>::pa_linear(q + K * i)]); });
            else {
                bool stored = false;
                if constexpr (WIDE_OUT) {
                    if (wide) { wide_tile_to_block<M>(out, base, X, q); stored = true; }
                }
                if (!stored) static_for<0, M>([&](auto ii) { constexpr int i = decltype(ii)::value; st_stream(out, base + q + K * i, X[q + K * i]); });
            }
        }
    }
    GFDM_STAMP(5);
