// The statements of the weight-streaming A16 tile (wq_stream_tile.h states the tile and why this is text, not a
// function): the body of wq_stream_kernel (wq.hip, MOE = false, m0 = x_rows = 0) and, after the expert walk, of
// moe_gemm_wq_wide_kernel (wq_moe_wide.hip, MOE = true).  Names read from the including kernel: the template parameters
// INT4, DT, ZP, MT; constexpr bool MOE; WqArgs p; int64_t m0 (first output row of the tile) and x_rows (rows of X).
// No include guard: it is included once per kernel.
    __shared__ f32x4 red[WQ_WAVES - 1][MT][64];
    // k-blocks in flight per wave: 32 VGPRs of weight chunks in either format
    constexpr int WQ_SB = INT4 ? 2 * WQ_UNROLL : WQ_UNROLL;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // in an SGPR: the k-block offsets are scalar
    const int r = lane & 15;            // A row (weight row n0 + r) and B column (activation row 16 t + r)
    const int kq = lane >> 4;           // which 32 columns of the k-block
    const int64_t n0 = (int64_t)blockIdx.x * 16;
    const int64_t n = n0 + r;
    const bool n_ok = n < p.N;
    const int64_t nrow = n_ok ? n : 0;
    const int nfull = p.K / WQ_KB;      // K is a multiple of WQ_KB
    const float off = INT4 ? 8.0f : 128.0f;
    constexpr int WV = INT4 ? 1 : 2;    // 16-byte weight chunks per lane per k-block
    // dense: the lane's byte offset in every m-tile's descriptor
    const int xoff = (int)(((int64_t)r * p.ldx + 32 * kq) * 2);
    // MOE: the lane's byte offset in the one descriptor over X, per m-tile; the descriptor's size for a dead row.  A
    // dead lane reads row_idx at the tile's first row (in bounds) and drops the value.
    const unsigned xsize = MOE ? (unsigned)((uint64_t)((x_rows - 1) * p.ldx + p.K) * 2) : 0u;
    unsigned xo[MOE ? MT : 1];
    if constexpr (MOE) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int m = 16 * t + r;
            const bool m_ok = m < p.M;
            const int64_t mm = m0 + (m_ok ? m : 0);
            int64_t row = mm;
            if (p.row_idx) row = min(max((int64_t)p.row_idx[mm], (int64_t)0), x_rows - 1);
            xo[t] = m_ok ? (unsigned)((uint64_t)(row * p.ldx + 32 * kq) * 2) : xsize;
        }
    }

    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    // UC k-blocks kb, kb + 4, ... of this wave: every weight load issued before the first MFMA
    auto batch = [&](const int kb, auto uc) {
        constexpr int UC = decltype(uc)::value;
        constexpr int STEPS = UC * MT;
        uint4 wv[UC][WV];
        u32x4 xv[WQ_XB][4];
        float sc[UC], cz[UC];
        // step i = (k-block u = i / MT, m-tile t = i % MT): its four 16-byte activation loads
        auto load_x = [&](int i, u32x4 (&dst)[4]) {
            const int u = i / MT, t = i % MT;
            if constexpr (MOE) {
                const int soff = (kb + u * WQ_WAVES) * (WQ_KB * 2);
                const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, (int)xsize, 0x00020000);
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    dst[s] = __builtin_bit_cast(
                        u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(xo[t] + 16 * s), soff, 0));
            } else {
                const int rows = min(p.M - 16 * t, 16);
                const auto rs = __builtin_amdgcn_make_buffer_rsrc(
                    (void*)(p.X + (int64_t)(16 * t) * p.ldx), 0, (int)(((int64_t)(rows - 1) * p.ldx + p.K) * 2),
                    0x00020000);
                const int soff = (kb + u * WQ_WAVES) * (WQ_KB * 2);
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    dst[s] =
                        __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, xoff + 16 * s, soff, 0));
            }
        };
#pragma unroll
        for (int i = 0; i < WQ_XB - 1 && i < STEPS; ++i) load_x(i, xv[i]);
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const int c0 = (kb + u * WQ_WAVES) * WQ_KB + 32 * kq;
            if constexpr (INT4) {
                const uint4* src = (const uint4*)((const int32_t*)p.Wq + nrow * p.Kw + c0 / 8);
                wv[u][0] = n_ok ? ld_nt16(src) : make_uint4(0x88888888u, 0x88888888u, 0x88888888u,
                                                                                 0x88888888u);
            } else {
                const uint4* src = (const uint4*)((const int8_t*)p.Wq + nrow * p.K + c0);
                wv[u][0] = n_ok ? ld_nt16(src) : make_uint4(0x80808080u, 0x80808080u, 0x80808080u,
                                                                                 0x80808080u);
                wv[u][1] = n_ok ? ld_nt16(src + 1)
                                : make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
            }
            float sv = 0.0f, czv = off;
            if (n_ok) group_params<INT4, ZP, false>(p, nrow, c0, sv, czv);
            sc[u] = sv;
            cz[u] = czv;
        }
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const float s = sc[u];
            const float noff = -(off * s);
            const unsigned wd[8] = {wv[u][0].x, wv[u][0].y, wv[u][0].z, wv[u][0].w, wv[u][WV - 1].x,
                                    wv[u][WV - 1].y, wv[u][WV - 1].z, wv[u][WV - 1].w};
            u32x4 a[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                float uu[8];
                if constexpr (INT4) u_int4(wd[s4], uu);
                else u_int8(wd[2 * s4], wd[2 * s4 + 1], uu);
                a[s4] = frag_from_u<DT, ZP>(uu, s, cz[u], noff);
            }
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const int i = u * MT + t;
                if (i + WQ_XB - 1 < STEPS) load_x(i + WQ_XB - 1, xv[(i + WQ_XB - 1) % WQ_XB]);
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) acc[t] = mfma16<DT>(a[s4], xv[i % WQ_XB][s4], acc[t]);
            }
        }
    };
    int kb = wave;
    int left = nfull > wave ? (nfull - wave + WQ_WAVES - 1) / WQ_WAVES : 0;   // this wave's k-blocks: kb, kb + 4, ...
    for (; left >= WQ_SB; left -= WQ_SB, kb += WQ_SB * WQ_WAVES) batch(kb, WqInt<WQ_SB>{});
    if constexpr (WQ_SB > 4) {
        if (left & 4) {
            batch(kb, WqInt<4>{});
            kb += 4 * WQ_WAVES;
        }
    }
    if (left & 2) {
        batch(kb, WqInt<2>{});
        kb += 2 * WQ_WAVES;
    }
    if (left & 1) batch(kb, WqInt<1>{});

    // as the skinny kernel, per m-tile: y = ((w0 + w1) + w2) + w3 (+ bias), one rounding
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < MT; ++t) red[wave - 1][t][lane] = acc[t];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int64_t m = 16 * t + r;
            f32x4 y4 = acc[t];
#pragma unroll
            for (int w = 0; w < WQ_WAVES - 1; ++w) {
                const f32x4 o = red[w][t][lane];
#pragma unroll
                for (int i = 0; i < 4; ++i) y4[i] = y4[i] + o[i];
            }
            if (m >= p.M) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t nn = n0 + 4 * kq + i;
                if (nn >= p.N) continue;
                float y = y4[i];
                if constexpr (MOE) {
                    p.Y[(m0 + m) * p.ldy + nn] = (unsigned short)(pack2<DT>(y, 0.0f) & 0xffffu);
                } else {
                    if (p.bias) y = y + h2f<DT>(p.bias[nn]);
                    p.Y[m * p.ldy + nn] = (unsigned short)(pack2<DT>(y, 0.0f) & 0xffffu);
                }
            }
        }
    }
