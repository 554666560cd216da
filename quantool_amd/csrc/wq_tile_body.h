// The statements of the 128 x 128 A16 tile (wq_tile.hip's head comment states the tile; wq_tile.h why this is text, not
// a function): the body of wq_tile_kernel (wq_tile.hip, MOE = false) behind its tile order and, behind the slot walk,
// of moe_gemm_wq_tile_kernel (wq_moe_tile.hip, MOE = true).  Names read from the including kernel: the template
// parameters INT4, DT, ZP; constexpr bool MOE; WqArgs p, one weight matrix [p.N, p.K] and the p.M rows it multiplies,
// row m to p.Y + m ldy; int m0, n0, the tile's first row and column.
//   MOE = false  row m is row m of p.X (row0 and x_rows are not read).
//   MOE = true   m0 = 0 and p.M <= 128, the live rows of the slot; row m is X[row_idx[row0 + m] clamped into
//                [0, x_rows)], or X[row0 + m] without row_idx (int64_t row0, x_rows).  The lane's four DMA offsets carry
//                the whole row address as 32-bit byte offsets from X itself (the host keeps x_rows ldx 2 + 2 K below
//                2^32); everything behind the offsets -- the loop, the LDS image, the fragment reads -- is the dense
//                kernel's, so a row has the dense kernel's bits.  No bias.
// No include guard: it is included once per kernel.
    constexpr int W_BYTES = TT * TKU / (INT4 ? 2 : 1);          // packed panel of a K-tile: 4 / 8 KiB
    constexpr int WI = INT4 ? 1 : 2;                            // its LDS-DMA instructions per wave
    constexpr int NI = 4 + WI + 1;                              // LDS-DMA instructions per wave and unit
    constexpr int SLOT_BYTES = TX_BYTES + W_BYTES + TS_BYTES;
    __shared__ __attribute__((aligned(16))) char lds[TSLOTS * SLOT_BYTES + 2 * TX_BYTES];
    char* ring = lds;
    char* img = lds + TSLOTS * SLOT_BYTES;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave_m = wave >> 1, wave_n = wave & 1;
    const int nt = p.K / TKU;                                   // K-tiles = phases, >= 2
    const int a_last = p.M - 1 - m0, b_last = p.N - 1 - n0;     // last valid row of each operand, relative to the tile
    const int wrow_b = p.K / (INT4 ? 2 : 1);                    // bytes of a packed weight row

    // ---- staging geometry: this lane's source byte offsets, relative to the K-tile's first byte in the tile's row 0 ----
    // (MOE: relative to the K-tile's first byte in row 0 of X)
    unsigned voffX[4], voffW, voffS;
#pragma unroll
    for (int i = 0; i < 4; ++i) {                               // row 32 wave + 8 i + (lane >> 3), physical chunk lane & 7
        const int r = 32 * wave + 8 * i + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        if constexpr (MOE) {                                    // a row past the live rows re-reads the last live row
            const int64_t mm = row0 + min(r, a_last);
            int64_t row = mm;
            if (p.row_idx) row = min(max((int64_t)p.row_idx[mm], (int64_t)0), x_rows - 1);
            voffX[i] = (unsigned)((uint64_t)(row * p.ldx) * 2 + 16 * c);
        } else {
            voffX[i] = (unsigned)((int64_t)min(r, a_last) * p.ldx * 2 + 16 * c);
        }
    }
    const int drow = 32 * wave + (lane >> 1);                   // the weight row this lane fetches and dequantises
    voffW = (unsigned)((int64_t)min(drow, b_last) * wrow_b + 16 * (lane & 1));     // int8: + 32 for the second piece
    const int scol = 64 * wave_n + lane;                        // the weight row whose scale / zero-point this lane fetches
    const bool zp_wave = ZP && wave_m;                          // waves 2, 3: the zero-points
    voffS = (unsigned)((int64_t)min(scol, b_last) * p.G * (zp_wave ? 1 : 4));
    const unsigned ring_lds = (unsigned)(size_t)(QT_LDS char*)ring;
    const unsigned dstX = __builtin_amdgcn_readfirstlane(ring_lds + wave * 4096);
    const unsigned dstW = __builtin_amdgcn_readfirstlane(ring_lds + TX_BYTES + wave * (1024 * WI));
    const unsigned dstS = __builtin_amdgcn_readfirstlane(ring_lds + TX_BYTES + W_BYTES + wave_m * 512 + wave_n * 256);
    const char* srcX = MOE ? (const char*)p.X : (const char*)(p.X + (int64_t)m0 * p.ldx);
    const char* srcW = (const char*)p.Wq + (int64_t)n0 * wrow_b;
    const char* srcS = zp_wave ? (const char*)p.zp_w + (int64_t)n0 * p.G : (const char*)p.s_w + (int64_t)n0 * p.G * 4;
    // unit u into `slot`: the X tile of K-tile u (none for u = -1) and the packed panel of K-tile min(u + 1, nt - 1)
    auto issue = [&](int u, int slot) {
        const unsigned off = (unsigned)slot * SLOT_BYTES;
        if (u >= 0) {
            const char* x = srcX + (size_t)u * (TKU * 2);
            glds16_pair(voffX[0], voffX[1], x, dstX + off, dstX + off + 1024);
            glds16_pair(voffX[2], voffX[3], x, dstX + off + 2048, dstX + off + 3072);
        }
        const int tw = min(u + 1, nt - 1);
        const char* w = srcW + (size_t)tw * (W_BYTES / TT);
        if constexpr (INT4) glds16_one(voffW, w, dstW + off);
        else glds16_pair(voffW, voffW + 32, w, dstW + off, dstW + off + 1024);
        const int g = p.G == 1 ? 0 : tw >> 1;
        if (zp_wave) glds1_one(voffS, srcS + g, dstS + off);
        else glds4_one(voffS, srcS + (size_t)g * 4, dstS + off);
    };

    // ---- fragment read geometry (per lane), byte offsets inside the X tile / the image ----
    const int lr = lane & 31, lh = lane >> 5;
    int xoff[4], woff[4];                                       // k-step s: chunk 2 s + lh; rows + 32: 4 pieces further
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        xoff[s] = tile_img(64 * wave_m + lr, 2 * s + lh);
        woff[s] = tile_img(64 * wave_n + lr, 2 * s + lh);
    }
    // ---- dequantise geometry: the lane's packed bytes, its scale, and where its four chunks go ----
    const int poff = TX_BYTES + wave * (1024 * WI) + 16 * lane; // int8: the second piece 1 KiB further
    const int soff = TX_BYTES + W_BYTES + 4 * drow;
    const bool drow_ok = drow <= b_last;
    const float off_u = INT4 ? 8.0f : 128.0f;
    int doff[4];                                                // chunk j of the lane's 32 weights
#pragma unroll
    for (int j = 0; j < 4; ++j)                                 // int4: columns 32 (lane & 1) + 8 j; int8: 16 ((lane & 1) + 2 (j >> 1)) + 8 (j & 1)
        doff[j] = tile_img(drow, INT4 ? 4 * (lane & 1) + j : 2 * ((lane & 1) + 2 * (j >> 1)) + (j & 1));

    unsigned pk[4 * WI];                                        // the lane's packed words of the K-tile being dequantised
    float dsc, dcz;
    auto load_packed = [&](const char* base) {
#pragma unroll
        for (int i = 0; i < WI; ++i) {
            const u32x4 v = *(const u32x4*)(base + poff + 1024 * i);
            pk[4 * i] = v.x, pk[4 * i + 1] = v.y, pk[4 * i + 2] = v.z, pk[4 * i + 3] = v.w;
        }
        const float s = *(const float*)(base + soff);
        dsc = drow_ok ? s : 0.0f;
        dcz = off_u;
        if constexpr (ZP) dcz = off_u + (float)(int)(signed char)(*(const int*)(base + soff + TT * 4) & 0xff);
    };
    // chunk j: 8 weights -> w = round_to_dtype((u - cz) s), 16 bytes into the image
    auto dequant_chunk = [&](int j, char* image) {
        float u[8];
        if constexpr (INT4) u_int4(pk[j], u);
        else u_int8(pk[2 * j], pk[2 * j + 1], u);
        float f[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float d = u[i] - dcz;
            f[i] = d * dsc;
        }
        *(u32x4*)(image + doff[j]) =
            (u32x4){pack2<DT>(f[0], f[1]), pack2<DT>(f[2], f[3]), pack2<DT>(f[4], f[5]), pack2<DT>(f[6], f[7])};
    };

    f32x16 acc[2][2];                                           // [nj][mi]: D rows = columns n, D columns = rows m
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nj][mi][r] = 0.0f;

    // slot = t % 3 and ib = t & 1 are scalars carried beside t: one copy of the phase
    auto phase = [&](int t, int slot, int ib) {
        if (t + 1 < nt) wait_vmcnt<NI>();                       // unit t has landed; unit t + 1 stays in flight
        else wait_vmcnt<0>();                                   // drain: the last unit
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");                          // no LDS access moves in front of the barrier
        if (t + TLEAD < nt) issue(t + TLEAD, slot == 0 ? TLEAD : slot - 1);     // (slot + 2) % 3
        const char* base = ring + slot * SLOT_BYTES;
        const char* wimg = img + ib * TX_BYTES;
        char* dimg = img + (ib ^ 1) * TX_BYTES;
        u32x4 fx[2][4], fw[2][4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                fw[h][s] = *(const u32x4*)(wimg + woff[s] + h * 4096);
                fx[h][s] = *(const u32x4*)(base + xoff[s] + h * 4096);
            }
        load_packed(base);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) acc[nj][mi] = tile_mfma<DT>(fw[nj][s], fx[mi][s], acc[nj][mi]);
            dequant_chunk(s, dimg);
        }
    };

    issue(-1, TSLOTS - 1);
    issue(0, 0);
    issue(1, 1);
    wait_vmcnt<2 * NI>();                                       // unit -1 has landed
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    load_packed(ring + (TSLOTS - 1) * SLOT_BYTES);
#pragma unroll
    for (int j = 0; j < 4; ++j) dequant_chunk(j, img);
    for (int t = 0, slot = 0; t < nt; ++t, slot = slot == TSLOTS - 1 ? 0 : slot + 1) phase(t, slot, t & 1);

    // ---- epilogue: y = acc (+ bias[n]), one rounding; element 4 j + i of (nj, mi) is column n + i of row m ----
    const bool has_bias = !MOE && p.bias != nullptr;
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nn = n0 + 64 * wave_n + 32 * nj + 8 * j + 4 * lh;
            if (nn >= p.N) continue;
            float b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = (has_bias && nn + i < p.N) ? h2f<DT>(p.bias[nn + i]) : 0.0f;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int64_t m = (int64_t)m0 + 64 * wave_m + 32 * mi + lr;
                if (m >= p.M) continue;
                float y[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    y[i] = acc[nj][mi][4 * j + i];
                    if (has_bias) y[i] = y[i] + b[i];
                }
                unsigned short* dst = p.Y + m * p.ldy + nn;
                if (p.vec && nn + 3 < p.N) {                    // vec: Y and its pitch are 8-byte aligned
                    *(uint2*)dst = make_uint2(pack2<DT>(y[0], y[1]), pack2<DT>(y[2], y[3]));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (nn + i < p.N) dst[i] = (unsigned short)(pack2<DT>(y[i], 0.0f) & 0xffffu);
                }
            }
        }
    }
