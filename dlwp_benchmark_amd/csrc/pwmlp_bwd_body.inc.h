// Body of the pointwise-MLP backward: the text of pwmlp_bwd_kernel<NIB, NOB, NW> (pwmlp.hip) and, with PWMLP_BWD_FUSED
// defined, the second phase of fno_spatial_lift_bwd_kernel (fno_block.hip), whose upstream gradient tile is already in LDS.
// Included as text, not called: a __device__ body that takes the argument block by reference cost every instantiation
// 1.1 us (profiles/r07_experiments.md).  Expects in scope: `a` (BwdArgs), `smem`, and the constants NIB, NOB, NW.
// PWMLP_BWD_FUSED drops what that launch never has: the staging of gy (MSE term, gres) and the fused rows DFT.  That launch
// includes the text in two parts (PWMLP_BWD_PART 1, then 2) around its `spatial` phase: part 1 ends where the loads that do not
// depend on the upstream gradient -- the wave's first weight fragments and, there, the first unit of the input tile through the
// pointer table -- have been requested, so their latency runs under the `spatial` phase (constant PWMLP_BWD_EARLY; false: they are
// requested at the start of part 2).
// PWMLP_BWD_BEHIND (without PWMLP_BWD_FUSED): the whole stand-alone text as the third phase of fno_spatial_lift_proj_bwd_kernel,
// behind another body in the same launch; it adds the one workgroup barrier in front of the first LDS store.
#if !defined(PWMLP_BWD_PART) || PWMLP_BWD_PART == 1
    constexpr bool SC = NOB == 0;
    constexpr int NB = SC ? 1 : NOB;         // 16-row output blocks of the slab layout and the operand arrays
    constexpr int NT = NW * 64;
#ifndef PWMLP_BWD_FUSED
    float* xs = smem;                        // [Cin_pad][LDP]
    float* gys = xs + a.Cin_pad * LDP;       // [Cout_pad][LDP]
    float* red = gys + a.Cout_pad * LDP;     // [NW][Cin_pad][LDP] gx partial tiles; later the rows-DFT table / partial spectra
#else
    float* gys = smem + a.Cout_pad * LDP;    // [Cout_pad][LDP]: the `spatial` phase's finished row (its tout_s; W == PT)
    float* xs = gys + a.Cout_pad * LDP;      // [Cin_pad][LDP]   over the `spatial` phase's dead regions
    float* red = xs + a.Cin_pad * LDP;       // [NW][Cin_pad][LDP]
#endif

    const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
    const int r = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / a.tiles_per_sample;
    const int p0 = (blockIdx.x % a.tiles_per_sample) * PT;

    const int nhb = a.Ch_pad / 16;
    const bool vec1 = a.vec_w != 0 && (a.Cin & 3) == 0;
    DLWP_STAMP(9);
    // weight fragments of one hidden block, straight from L2: W1 rows (B operand of z^T), b1, W2 columns of the block (B operand
    // of g_a^T), W1 columns (A operand of dX).  A wave owns its hidden blocks alone, so every fragment is read once per workgroup.
    struct HbW {
        f32x4 w1b[NIB], w2c[NB], w1c[NIB];
        float b1v, w2v;               // w2v (SC): W2[0][hb*16 + r]
    };
    auto load_hb = [&](int hb, HbW& h) {
#pragma unroll
        for (int kc = 0; kc < NIB; ++kc) h.w1b[kc] = frag_row(a.w1, a.Ch, a.Cin, hb * 16 + r, kc * 16 + 4 * g, vec1);
        if constexpr (!SC) {
#pragma unroll
            for (int oc = 0; oc < NB; ++oc) h.w2c[oc] = frag_col(a.w2, a.Cout, a.Ch, oc * 16 + 4 * g, hb * 16 + r);
        }
#pragma unroll
        for (int ib = 0; ib < NIB; ++ib) h.w1c[ib] = frag_col(a.w1, a.Ch, a.Cin, hb * 16 + 4 * g, ib * 16 + r);
        const bool okh = hb * 16 + r < a.Ch;
        const float bv = a.b1[okh ? hb * 16 + r : 0];
        h.b1v = okh ? bv : 0.f;
        if constexpr (SC) {
            const float wv = a.w2[okh ? hb * 16 + r : 0];
            h.w2v = okh ? wv : 0.f;
        }
    };
    HbW wcur;
#ifndef PWMLP_BWD_FUSED
    load_hb(w < nhb ? w : 0, wcur);                        // in flight while the pixel tiles are staged
#else
    // the wave's first weight fragments and the first 16-byte unit of this thread's share of the input tile (stage_pixels' unit
    // u = tid; committed to xs in part 2) in front of the `spatial` phase where the registers allow (PWMLP_BWD_EARLY); else both
    // are requested in part 2, the tile by stage_pixels
    const int xu_c = tid / (PT / 4), xu_q = tid % (PT / 4);
    float4 xu_v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (PWMLP_BWD_EARLY) {
        load_hb(w < nhb ? w : 0, wcur);
        if (a.vec_x && xu_c < a.Cin && p0 + 4 * xu_q < a.P) {
            const float* src = chan_ptr(a.x, b, xu_c);
            if (src) xu_v = *reinterpret_cast<const float4*>(src + p0 + 4 * xu_q);
        }
    }
#endif
#endif
#if !defined(PWMLP_BWD_PART) || PWMLP_BWD_PART == 2
#ifdef PWMLP_BWD_FUSED
    if (!PWMLP_BWD_EARLY) load_hb(w < nhb ? w : 0, wcur);
#endif
#ifndef PWMLP_BWD_FUSED
    float4 ftv = make_float4(0.f, 0.f, 0.f, 0.f);          // DFT table [16][PT] of the fused rows step
    if (a.x1_out && tid < 16 * (PT / 4)) ftv = reinterpret_cast<const float4*>(a.FT)[tid];
#endif
#ifdef PWMLP_BWD_BEHIND
    // third phase of fno_spatial_lift_proj_bwd_kernel: the LDS below is the lifting phase's until here, and the upstream gradient
    // rows staged below are the ones this workgroup has just accumulated in global memory.  The weight fragments and the table
    // requested above depend on neither.
    __syncthreads();
#endif
#ifndef PWMLP_BWD_FUSED
    stage_pixels(xs, a.x, b, a.Cin, a.Cin_pad, p0, a.P, a.vec_x != 0);
    const bool has_gy = a.gy.base || a.gy.tab;
    const bool has_mse = a.pred.base || a.pred.tab;
    if (has_gy && !has_mse) {
        stage_pixels(gys, a.gy, b, a.Cout, a.Cout_pad, p0, a.P, a.vec_x != 0);
    } else {
        for (int idx = tid; idx < a.Cout_pad * PT; idx += NT) {
            const int c = idx / PT, p = idx % PT;
            float v = 0.f;
            if (c < a.Cout && p0 + p < a.P) {
                if (has_gy) {
                    const float* src = chan_ptr(a.gy, b, c);
                    if (src) v = src[p0 + p];
                }
                if (has_mse) {
                    const float* pp = chan_ptr(a.pred, b, c);
                    const float* tp = chan_ptr(a.target, b, c);
                    v += a.mse_scale * (pp[p0 + p] - tp[p0 + p]);
                }
            }
            gys[c * LDP + p] = v;
        }
    }
    __syncthreads();
    if (a.gres.base || a.gres.tab) {
        for (int idx = tid; idx < a.Cout * PT; idx += NT) {
            const int o = idx / PT, p = idx % PT;
            float* dst = chan_ptr(a.gres, b, o);
            if (dst && p0 + p < a.P) dst[p0 + p] += gys[o * LDP + p];
        }
    }
#else
    if (PWMLP_BWD_EARLY && a.vec_x) {
        if (xu_c < a.Cin_pad) *reinterpret_cast<float4*>(&xs[xu_c * LDP + 4 * xu_q]) = xu_v;
        for (int u = tid + NT; u < a.Cin_pad * (PT / 4); u += NT) {       // more than NT units: Cin_pad > 32
            const int c = u / (PT / 4), q = u % (PT / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < a.Cin && p0 + 4 * q < a.P) {
                const float* src = chan_ptr(a.x, b, c);
                if (src) v = *reinterpret_cast<const float4*>(src + p0 + 4 * q);
            }
            *reinterpret_cast<float4*>(&xs[c * LDP + 4 * q]) = v;
        }
    } else {
        stage_pixels(xs, a.x, b, a.Cin, a.Cin_pad, p0, a.P, !PWMLP_BWD_EARLY && a.vec_x != 0);
    }
    __syncthreads();
#endif

    DLWP_STAMP(10);

    // wave-private 16 x 16 transpose tile (gz^T -> gz) inside the gx partial-tile region, which is idle until the main loop ends
    static_assert(16 * TPS <= 16 * LDP, "a wave's transpose tile fits into its own partial-tile rows");
    float* tp = red + w * 16 * TPS;

    f32x4 gxacc[4][NIB];
#pragma unroll
    for (int pb = 0; pb < 4; ++pb)
#pragma unroll
        for (int ib = 0; ib < NIB; ++ib) gxacc[pb][ib] = f32x4{0.f, 0.f, 0.f, 0.f};
    float* sl = a.slab ? a.slab + (long long)blockIdx.x * a.slab_stride : nullptr;
    // slab layout per workgroup: [nhb][NB][64][4] dW2 tiles | [nhb][NIB][64][4] dW1 tiles | db1[Ch_pad] | db2[Cout_pad]
    const long long o_t1 = (long long)(a.Ch_pad / 16) * NB * 256, o_gb1 = o_t1 + (long long)(a.Ch_pad / 16) * NIB * 256;
    const long long o_gb2 = o_gb1 + a.Ch_pad;
    const bool accum = sl && a.slab_accumulate != 0;
    DLWP_STAMP(11);
    // Everything below works in the TRANSPOSED orientation (rows = pixels 4g+j, column = hidden channel r):
    // the accumulator of z^T / gz^T is then directly the B operand of the pixel contractions (dW2) and, read as an
    // A operand, the hidden-major matrix for dW1; the one product that contracts over the hidden index (dX) gets
    // its operand through a wave-private LDS transpose (no workgroup barrier).
    // One hidden block's state while its four pixel blocks are processed.
    struct HbState {
        f32x4 pgw2[NB], pgw1[NIB];   // running slab partials (read-modify-write accumulation across net calls)
        float pgb1;
        f32x4 gw2acc[NB], gw1acc[NIB];
        float gb1acc;
        float *t2, *t1;
        int hb;
    };
    auto hb_begin = [&](HbState& st, int hb) {
        st.hb = hb;
        // The slab is private scratch, so it is laid out in ACCUMULATOR-TILE order: tile (hb, ob) holds the 4
        // registers of every lane contiguously -> one 16-byte access per lane, 1 KiB per wave-instruction
        // (narrow 64-byte-segment stores were issue-bound: ~350 cycles each).  The old values are fetched here.
        st.pgb1 = 0.f;
        st.t2 = sl ? sl + ((long long)hb * NB * 64 + lane) * 4 : nullptr;
        st.t1 = sl ? sl + o_t1 + ((long long)hb * NIB * 64 + lane) * 4 : nullptr;
#pragma unroll
        for (int ob = 0; ob < NB; ++ob)
            st.pgw2[ob] = accum ? *reinterpret_cast<const f32x4*>(st.t2 + ob * 256) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ib = 0; ib < NIB; ++ib)
            st.pgw1[ib] = accum ? *reinterpret_cast<const f32x4*>(st.t1 + ib * 256) : f32x4{0.f, 0.f, 0.f, 0.f};
        if (accum && g == 0) st.pgb1 = sl[o_gb1 + hb * 16 + r];
        st.gb1acc = 0.f;
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) st.gw2acc[ob] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ib = 0; ib < NIB; ++ib) st.gw1acc[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // One pixel block in two stages, software-pipelined by the caller: stage A (z^T and g_a^T, MFMA only) of block pb + 1 is
    // issued in front of stage B (GELU on the VALU, then the products that need it) of block pb, and the k-steps of
    // independent accumulators are interleaved (a 16x16x4 MFMA that accumulates into its predecessor's result issues every 40
    // cycles instead of 32).  Measured: neither changes the kernel (22.4 / 20.4 us before and after) -- on one SIMD the exact-f32
    // MFMA and ordinary VALU instructions do not co-execute at all (tools/micro/mfma_valu_coexec.hip: 257 k + 177 k cycles
    // apart, 433 k together), so the main loop costs MFMA cycles PLUS GELU cycles however they are ordered.
    auto hb_stage_a = [&](const HbW& hw, int pb, f32x4& zt, f32x4& gat) {
        // z^T[p][h] = sum_i x[i][p] W1[h][i];  g_a^T[p][h] = sum_o gy[o][p] W2[o][h]
        f32x4 az[NIB];
#pragma unroll
        for (int kc = 0; kc < NIB; ++kc)
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) az[kc][s2] = xs[(kc * 16 + 4 * g + s2) * LDP + pb * 16 + r];
        zt = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (SC) {
#pragma unroll
            for (int c = 0; c < NIB; ++c)
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2) zt = mfma16(az[c][s2], hw.w1b[c][s2], zt);
            // one 16-byte read of the gy row: pixels pb*16 + 4g .. + 3
            gat = *reinterpret_cast<const f32x4*>(&gys[pb * 16 + 4 * g]) * f32x4{hw.w2v, hw.w2v, hw.w2v, hw.w2v};
        } else {
            f32x4 ag[NB];
#pragma unroll
            for (int oc = 0; oc < NB; ++oc)
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2) ag[oc][s2] = gys[(oc * 16 + 4 * g + s2) * LDP + pb * 16 + r];
            gat = f32x4{0.f, 0.f, 0.f, 0.f};
            constexpr int NMAX = NIB > NB ? NIB : NB;
#pragma unroll
            for (int c = 0; c < NMAX; ++c)
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2) {
                    if (c < NIB) zt = mfma16(az[c][s2], hw.w1b[c][s2], zt);
                    if (c < NB) gat = mfma16(ag[c][s2], hw.w2c[c][s2], gat);
                }
        }
    };
    auto hb_stage_b = [&](HbState& st, const HbW& hw, int pb, const f32x4 zt, const f32x4 gat) {
        f32x4 actt, gzt, dvt;
        gelu_both4(zt + f32x4{hw.b1v, hw.b1v, hw.b1v, hw.b1v}, actt, dvt);      // packed fp32 polynomial
        gzt = gat * dvt;
        st.gb1acc += (gzt[0] + gzt[1]) + (gzt[2] + gzt[3]);
        // dW2[o][h] += sum_p gy[o][p] act^T[p][h];  dW1[h][i] += sum_p gz[h][p] x[i][p]  (gz^T registers read as an A operand
        // are gz)
        // gz[h][p] in accumulator layout is the 16 x 16 transpose of gz^T: through the wave's own LDS tile (row h = r gets this
        // lane's four pixels, then column reads), not through the matrix pipe -- a product with the identity was 4 of the
        // block's MFMAs, 128 issue cycles against ~30 here; the dW2 / dW1 products below do not need gz and cover the round trip
        f32x4 gz;
        wave_lds_order();
        *reinterpret_cast<f32x4*>(&tp[r * TPS + 4 * g]) = gzt;
        wave_lds_order();
#pragma unroll
        for (int j = 0; j < 4; ++j) gz[j] = tp[(4 * g + j) * TPS + r];
        f32x4 a2[NB], b1f[NIB];
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) a2[ob] = *reinterpret_cast<const f32x4*>(&gys[(ob * 16 + r) * LDP + pb * 16 + 4 * g]);
#pragma unroll
        for (int ib = 0; ib < NIB; ++ib) b1f[ib] = *reinterpret_cast<const f32x4*>(&xs[(ib * 16 + r) * LDP + pb * 16 + 4 * g]);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
#pragma unroll
            for (int ob = 0; ob < NB; ++ob) st.gw2acc[ob] = mfma16(a2[ob][s2], actt[s2], st.gw2acc[ob]);
#pragma unroll
            for (int ib = 0; ib < NIB; ++ib) st.gw1acc[ib] = mfma16(gzt[s2], b1f[ib][s2], st.gw1acc[ib]);
        }
        // dX[i][p] += sum_h W1[h][i] gz[h][p]
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
            for (int ib = 0; ib < NIB; ++ib) gxacc[pb][ib] = mfma16(hw.w1c[ib][s2], gz[s2], gxacc[pb][ib]);
    };
    auto hb_flush = [&](HbState& st) {
        const int hb = st.hb;
        if (sl) {
#pragma unroll
            for (int ob = 0; ob < NB; ++ob) {
                f32x4 v = st.gw2acc[ob];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] += st.pgw2[ob][j];
                *reinterpret_cast<f32x4*>(st.t2 + ob * 256) = v;
            }
#pragma unroll
            for (int ib = 0; ib < NIB; ++ib) {
                f32x4 v = st.gw1acc[ib];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] += st.pgw1[ib][j];
                *reinterpret_cast<f32x4*>(st.t1 + ib * 256) = v;
            }
        } else {
            const int hcol = hb * 16 + r;
#pragma unroll
            for (int ob = 0; ob < NB; ++ob)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int o = ob * 16 + 4 * g + j;
                    if (o < a.Cout && hcol < a.Ch) atomic_add_f32(a.gw2 + o * a.Ch + hcol, st.gw2acc[ob][j]);
                }
#pragma unroll
            for (int ib = 0; ib < NIB; ++ib)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int h = hb * 16 + 4 * g + j, i = ib * 16 + r;
                    if (h < a.Ch && i < a.Cin) atomic_add_f32(a.gw1 + h * a.Cin + i, st.gw1acc[ib][j]);
                }
        }
        float v = st.gb1acc;                       // bias gradient of hidden channel hb*16 + r: sum the 4 lane groups
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        const int h = hb * 16 + r;
        if (g == 0) {
            if (sl) sl[o_gb1 + h] = st.pgb1 + v;
            else if (h < a.Ch) atomic_add_f32(a.gb1 + h, v);
        }
    };
    {
        // Two waves share each SIMD's matrix pipe; in-kernel stamps showed waves 0-3 leaving this loop after 20 k cycles and
        // waves 4-7 after 29 k, with the barrier behind it waiting for the slowest.  The younger half runs the FIRST half of
        // its hidden blocks at raised priority and the second half at the default (moves the skew by < 2 k cycles).
        const int hb_half = w + NW * (((nhb - w + NW - 1) / NW) / 2);     // first hidden block of this wave's second half
        if (w >= NW / 2) __builtin_amdgcn_s_setprio(1);
        for (int hb = w; hb < nhb; hb += NW) {
            if (w >= NW / 2 && hb == hb_half) __builtin_amdgcn_s_setprio(0);
            HbState st;
            hb_begin(st, hb);
            if (hb == w) DLWP_STAMP(12);
            f32x4 zt, gat;
            hb_stage_a(wcur, 0, zt, gat);
#pragma unroll
            for (int pb = 0; pb < 4; ++pb) {
                f32x4 ztn = zt, gatn = gat;
                if (pb < 3) hb_stage_a(wcur, pb + 1, ztn, gatn);
                hb_stage_b(st, wcur, pb, zt, gat);
                zt = ztn; gat = gatn;
            }
            if (hb == w) DLWP_STAMP(18);
            // the next block's fragments are requested here, behind the last use of the current ones: their latency overlaps the
            // slab stores and the next hb_begin, and they add no live registers to the pixel-block loop
            if (hb + NW < nhb) load_hb(hb + NW, wcur);
            hb_flush(st);
            if (hb == w) DLWP_STAMP(19);
        }
    }
    __builtin_amdgcn_s_setprio(0);
    DLWP_STAMP(20);
    DLWP_STAMP_WAVE(24);      // end of every wave's main loop (slots 24..31)
    // cross-wave reduction of gx: every wave parks its [Cin_pad][64] partial tile in LDS (the weight
    // images are dead by now and are reused), then all threads sum the NW tiles.  (LDS float atomics
    // run at <1 lane-op per clock per CU on gfx950 and were the slowest phase of this kernel.)
    const bool want_gx = a.gx.base || a.gx.tab;
    DLWP_STAMP(20);
    __syncthreads();
    if (want_gx) {
#pragma unroll
        for (int pb = 0; pb < 4; ++pb)
#pragma unroll
            for (int ib = 0; ib < NIB; ++ib)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    red[(w * a.Cin_pad + ib * 16 + 4 * g + j) * LDP + pb * 16 + r] = gxacc[pb][ib][j];
    }
    DLWP_STAMP(21);
    __syncthreads();
    DLWP_STAMP(22);
    if (want_gx) {
        for (int u = tid; u < a.Cin * (PT / 4); u += NT) {
            const int c = u / (PT / 4), q = u % (PT / 4), p = p0 + 4 * q;
            float* dst = chan_ptr(a.gx, b, c);
            if (dst && p < a.P) {
                float4 v = *reinterpret_cast<const float4*>(&red[c * LDP + 4 * q]);
#pragma unroll
                for (int w2 = 1; w2 < NW; ++w2) {
                    const float4 pv = *reinterpret_cast<const float4*>(&red[(w2 * a.Cin_pad + c) * LDP + 4 * q]);
                    v.x += pv.x; v.y += pv.y; v.z += pv.z; v.w += pv.w;
                }
                if (a.vec_x) {
                    float4* d4 = reinterpret_cast<float4*>(dst + p);
                    if (a.gx_accumulate) { const float4 o = *d4; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                    *d4 = v;
                    if (a.x1_out) *reinterpret_cast<float4*>(&xs[c * LDP + 4 * q]) = v;   // finished row tile (x is dead)
                } else {
                    const float vv[4] = {v.x, v.y, v.z, v.w};
                    for (int k = 0; k < 4; ++k)
                        if (p + k < a.P) dst[p + k] = a.gx_accumulate ? dst[p + k] + vv[k] : vv[k];
                }
            }
        }
    }
    if (tid < a.Cout) {
        float s = 0.f;
        for (int p = 0; p < PT; ++p) s += gys[tid * LDP + p];
        grad_flush(sl ? sl + o_gb2 + tid : nullptr, a.gb2 + tid, accum, s);
    }
#ifndef PWMLP_BWD_FUSED
    if (a.x1_out) {
        // W-axis pruned DFT of the finished gradient row.  The partial-tile region is dead after the barrier: it hosts the
        // table and the per-wave partial spectra.
        __syncthreads();
        float* x1s = red;                          // [4 waves][Cin_pad][16]
        float* ft = red + 4 * a.Cin_pad * 16;      // [16][LDP]
        if (tid < 16 * (PT / 4)) *reinterpret_cast<float4*>(&ft[(tid / (PT / 4)) * LDP + 4 * (tid % (PT / 4))]) = ftv;
        for (int idx = a.Cin * LDP + tid; idx < a.Cin_pad * LDP; idx += NT) xs[idx] = 0.f;
        __syncthreads();
        if (w < 4) tile_rows_dft<NIB, 1>(xs, ft, x1s, LDP, 16, PT / 16, false);
        __syncthreads();
        store_x1(x1s, a.x1_out, b, (int)(blockIdx.x % a.tiles_per_sample), a.rows_H, a.m2c, a.Cin, a.Cin_pad, 16);
    }
#endif
    DLWP_STAMP(23);
#endif
