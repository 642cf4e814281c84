// Head of the two-role backward `spatial` workgroup, up to and including its second barrier (tout_s complete, role B finished):
// the text of fno_spatial_roles_kernel<NCB, NBN, MODE> and the first phase of fno_spatial_lift_bwd_kernel (both fno_block.hip).
// Included as text.  Expects in scope: `a` (SpatialDev), `smem`, and the constants NCB, NBN, MODE, ROLE_B.  ROLE_B == false: the
// by-products were formed elsewhere (fno_mix_bwd_skipgrad_kernel); waves 4-7 touch neither `pprev` nor the slab and only arrive
// at the barriers.
    constexpr int NTA = SPATIAL_NT;               // threads of role A (and of role B)
    constexpr bool need_prev = ROLE_B || MODE == 1;   // pprev feeds role B and the GELU' epilogue only
    const SpatialLds L = carve_spatial_lds<true>(smem, a);
    const int tid = threadIdx.x, lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(wave_id());   // wave-uniform: the role branches are scalar branches
    const bool role_a = w < 4;
    const int tb = tid - NTA, w2 = w - 4;         // role B's thread / wave index
    const int r = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
    const int W4 = a.W / 4, nwb = a.W / 16;
    DLWP_SPAN_BEGIN();
    DLWP_STAMP(0);
    // ---- issue phase (role A: the chain's; role B: the running partials of this workgroup's gradient slab)
    SpatialLoads R;
    constexpr int SLQ = 4;
    float slab_old[SLQ], slab_b_old = 0.f;
#pragma unroll
    for (int k = 0; k < SLQ; ++k) slab_old[k] = 0.f;
    const long long slab_off = spatial_slab_off(a);
    const bool slab_acc = a.gslab && a.gslab_accumulate;
    const int bias_c = 4 * lane + w2;             // role B: bias-gradient channel of this lane (lanes 0-15 of each wave)
    constexpr int BQ = 16;                        // ... its row pieces read ahead (a whole row at W = 64)
    const bool bias_on = !role_a && (a.g_bias || a.gslab) && lane < 16 && bias_c < a.C;
    if (role_a) {
        spatial_issue<MODE>(a, b, h, need_prev, R);
    } else if constexpr (ROLE_B) {
        if (slab_acc) {
#pragma unroll
            for (int k = 0; k < SLQ; ++k) slab_old[k] = a.gslab[slab_off + min(tb + NTA * k, a.C * a.C - 1)];
            slab_b_old = a.gslab[slab_off + a.C * a.C + min(bias_c, a.C - 1)];
        }
        // gK partial of wave w2: sum over its 16-pixel chunks of g_pre[o][w] * act(x)[i][w].  The MFMA fragments are 16 contiguous
        // bytes of a row of `tin` / `pprev`: they come straight from global memory (the values role A is putting into tin_s /
        // pprev_s; rows >= C are zero there), so this GEMM runs while role A waits for its own loads, not next to the main GEMM
        f32x4 kacc[NCB][NCB];
#pragma unroll
        for (int ob = 0; ob < NCB; ++ob)
#pragma unroll
            for (int ib = 0; ib < NCB; ++ib) kacc[ob][ib] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kc = w2; kc < nwb; kc += 4) {
            f32x4 ta[NCB], pb[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {   // clamped addresses, selects afterwards: all loads in flight together
                const int c = cb * 16 + r;
                const long long off = (((long long)b * a.C + min(c, a.C - 1)) * a.H + h) * a.W + kc * 16 + 4 * g;
                ta[cb] = *reinterpret_cast<const f32x4*>(&a.tin[off]);
                pb[cb] = *reinterpret_cast<const f32x4*>(&a.pprev[off]);
            }
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const bool ok = cb * 16 + r < a.C;
                ta[cb] = ok ? ta[cb] : f32x4{0.f, 0.f, 0.f, 0.f};
                pb[cb] = ok ? pb[cb] : f32x4{0.f, 0.f, 0.f, 0.f};
                if (a.act_tin) ta[cb] = gelu4(ta[cb]);
            }
#pragma unroll
            for (int ib = 0; ib < NCB; ++ib) {
                f32x4 b4 = pb[ib];
                if (a.act_prev) {
                    b4 = gelu4(b4);
                }
#pragma unroll
                for (int ob = 0; ob < NCB; ++ob) kacc[ob][ib] = mfma16_chunk(ta[ob], b4, kacc[ob][ib]);
            }
        }
#pragma unroll
        for (int ob = 0; ob < NCB; ++ob)
#pragma unroll
            for (int ib = 0; ib < NCB; ++ib)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    L.gks[((w2 * NCB + ob) * 16 + 4 * g + j) * a.C_pad + ib * 16 + r] = kacc[ob][ib][j];
        DLWP_STAMP_IF(blockIdx.x == 0 && tb == 0, 13);
    }
    DLWP_STAMP(1);

    if (role_a) {
        spatial_commit<MODE>(a, L, b, h, need_prev, R);
        DLWP_STAMP(3);
        spatial_hstep(a, L, b, h, R);
        DLWP_STAMP(4);
    }
    __syncthreads();   // 1: tin_s, pprev_s, gs, ks, s1 complete (role A); the four gK partials complete (role B)
    DLWP_STAMP(5);

    if (role_a) {
        spatial_gemm<NCB, NBN, MODE>(a, L, w);
        DLWP_STAMP(6);
    } else if constexpr (ROLE_B) {
        // cross-wave sum of the gK partials (w2 = 0 .. 3 from 0.f), then old + v into the slab, or the atomics.  The first SLQ
        // elements of a thread: all LDS reads first, then the sums (a read-then-use loop pays the LDS latency per element)
        // Bias gradient: channel 4 lane + w2 on lanes 0-15 of every wave, its row of tin_s as 16-byte reads (the first BQ issued
        // here, in front of the sums), additions in the order x = 0 .. W-1 from 0.f.
        const float4* brow = reinterpret_cast<const float4*>(&L.tin_s[min(bias_c, a.C_pad - 1) * L.LDP]);
        float4 bq[BQ];
        if (bias_on) {
#pragma unroll
            for (int q = 0; q < BQ; ++q) bq[q] = brow[min(q, W4 - 1)];
        }
        float pq[SLQ][4];
#pragma unroll
        for (int k = 0; k < SLQ; ++k) {
            const int idx = min(tb + NTA * k, a.C * a.C - 1), o = fastdiv(idx, a.dC), i = idx - o * a.C;
#pragma unroll
            for (int q = 0; q < 4; ++q) pq[k][q] = L.gks[(q * a.C_pad + o) * a.C_pad + i];
        }
#pragma unroll
        for (int k = 0; k < SLQ; ++k) {
            const int idx = tb + NTA * k;
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) v += pq[k][q];
            if (idx < a.C * a.C) spatial_flush(a, slab_off + idx, &a.g_wskip[idx], slab_old[k], v);
        }
        for (int idx = tb + NTA * SLQ; idx < a.C * a.C; idx += NTA) {
            const int o = fastdiv(idx, a.dC), i = idx - o * a.C;
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) v += L.gks[(q * a.C_pad + o) * a.C_pad + i];
            spatial_flush(a, slab_off + idx, &a.g_wskip[idx], slab_acc ? a.gslab[slab_off + idx] : 0.f, v);
        }
        if (bias_on) {
            float bias_sum = 0.f;
#pragma unroll
            for (int q = 0; q < BQ; ++q)
                if (q < W4) { bias_sum += bq[q].x; bias_sum += bq[q].y; bias_sum += bq[q].z; bias_sum += bq[q].w; }
            for (int x4 = BQ; x4 < W4; ++x4) {
                const float4 v = brow[x4];
                bias_sum += v.x; bias_sum += v.y; bias_sum += v.z; bias_sum += v.w;
            }
            spatial_flush(a, slab_off + a.C * a.C + bias_c, &a.g_bias[bias_c], slab_b_old, bias_sum);
        }
        DLWP_STAMP_IF(blockIdx.x == 0 && tb == 0, 15);
    }
    // 2: tout_s complete.  Role B is finished: it touches no LDS behind this barrier and must not wait for its slab stores in
    // front of one (__syncthreads() is a fence as well: vmcnt(0)); it only arrives, here and at the third.
    if (role_a) __syncthreads(); else __builtin_amdgcn_s_barrier();
    DLWP_STAMP(7);
