// gvl_paint_chunk.inc -- the body of realign_paint_kernel's chunk-wave, (row k, chunk) of n_chunks; included by realign_paint_kernel
// (the rows x chunks grid) and realign_paint_list_kernel (ragged rows' chunk list), gvl_tracks_kernels.inc.  In scope there: A, the
// LDS tables mirror[4] / wins[4], lane, wave, k, chunk, n_chunks and PAINT_STAMP.
#ifdef GVL_DIAG
    const bool tl_on = A.stamps != nullptr && (A.dbg & DBG_PAINT_TIMELINE) != 0;
#endif
    PAINT_STAMP(0);
    const u64 kernarg = (u64)__builtin_amdgcn_kernarg_segment_ptr();
    typedef const int __attribute__((address_space(4))) *KInt;
    typedef const i64 __attribute__((address_space(4))) *KI64;
    PaintWin &W = wins[wave];
    bool fast = A.plan_hdr != nullptr && A.plan_ent != nullptr && !(A.dbg & (DBG_SCALAR_WALK | DBG_NO_TRACK_PLANS | DBG_NO_REALIGN_WINDOW)) && A.out_offsets != nullptr;
    // ---- head: what the row's number alone addresses, one round of scalar loads (no shift, genotype slot or keep mask: the plan holds the walk)
    const i64 query = A.ploidy_shift >= 0 ? (k >> A.ploidy_shift) : (i64)((u32)k / (u32)A.ploidy);
    int ph_first = 0, ph_count = -1;
    i64 row_base = 0, row_end = 0, t_s = 0, t_e = 0, idx_raw = 0;
    int q_start = 0, rc_word = 0;
    const u64 rc_addr = (u64)A.to_rc + (u64)k;
    if (fast) {
#if defined(__HIP_DEVICE_COMPILE__)
        const PaintSrcArgsK PSk = (PaintSrcArgsK)(kernarg + sizeof(TrackArgs));
        const i64 *const oi_ptr = PSk->offset_idxs;
        const KInt w = (KInt)(u64)(A.plan_hdr + (k * (i64)n_chunks + (i64)chunk));
        ph_first = w[0]; ph_count = w[1];
        row_base = ((KI64)(u64)A.out_offsets)[k]; row_end = ((KI64)(u64)A.out_offsets)[k + 1];
        t_s = ((KI64)(u64)A.track_offsets)[query << A.to_shift]; t_e = ((KI64)(u64)A.track_offsets)[(query << A.to_shift) + 1];
        q_start = ((KInt)(u64)A.regions)[query * A.regions_stride + 1];
        rc_word = A.to_rc ? ((KInt)(rc_addr & ~3ull))[0] : 0;
        idx_raw = ((KI64)(u64)oi_ptr)[query];
        asm volatile("" :: "s"(ph_first), "s"(ph_count), "s"(row_base), "s"(row_end), "s"(t_s), "s"(t_e), "s"(q_start), "s"(rc_word), "s"(idx_raw));
#endif
    }
    const i64 L64 = row_end - row_base, tlen = t_e - t_s;
    fast = fast && ph_count > 0 && ph_count <= SEG_CAP && L64 > 0 && L64 < 0x7FFFFF00ll && tlen > 0 && tlen < 0x7FFFFF00ll &&
           q_start > -(1 << 30) && q_start < (1 << 30);
    const int L = (int)L64;
    const int lo_clip = chunk * A.chunk_len;
    if (fast && lo_clip >= L) return;
    const int hi_clip = (L - lo_clip > A.chunk_len) ? lo_clip + A.chunk_len : L;
    // ---- the chunk's entries, lane t = entry t: {first output position, kind, delta (runs) or position (repeats), -}
    const int nseg = fast ? ph_count : 0;
    const bool ev = lane < nseg;
    int e_out = 0x7FFFFFFF, e_kind = T_ZERO, e_plo = 0;
    if (fast && ev) {
        const i32x4 e = A.plan_ent[k * (i64)PLAN_MAXE + ph_first + lane];
        e_out = e.x; e_plo = e.z;
        e_kind = (e.y == T_FILL && A.strategy == GVL_FILL_REPEAT_5P) ? (int)T_REPEAT : e.y;
    }
    if (fast && __builtin_amdgcn_ballot_w64(ev && e_kind != T_TRACK && e_kind != T_REPEAT && e_kind != T_ZERO) != 0) fast = false;   // per-position fills
    // ---- the window: from where the chunk's first value comes from on
    i64 x_lo = 0; int wlen = 0;
    if (fast) {
#if defined(__HIP_DEVICE_COMPILE__)
        const PaintSrcArgsK PS = (PaintSrcArgsK)(kernarg + sizeof(TrackArgs));
        const i64 dv = PS->list_div;
        const i64 idx = dv == 1 ? idx_raw : rfl64(idx_raw / dv);
        const int k0 = rdl(e_kind, 0), p0v = rdl(e_plo, 0);
        fast = paint_build_window(W, PS, idx, (i64)q_start, tlen, k0 == T_TRACK ? (i64)p0v + lo_clip : (i64)p0v, lane, x_lo, wlen);
#endif
    }
    PAINT_STAMP(3);
    // ---- every source position the chunk reads lies inside the window and the track: entry t covers output [max(start, lo_clip),
    // min(next start, hi_clip)); a run reads track positions delta + those, a repeat one position
    if (fast) {
        const int nxt = bperm(lane + 1 < WAVE ? lane + 1 : WAVE - 1, e_out);          // lane t + 1's first output position
        const int o0 = e_out < lo_clip ? lo_clip : e_out;
        int o1 = (lane + 1 < nseg ? nxt : hi_clip);
        o1 = o1 > hi_clip ? hi_clip : o1;
        bool okc = true;
        if (ev && o1 > o0) {
            const i64 xa = e_kind == T_TRACK ? (i64)e_plo + o0 : (i64)e_plo, xb = e_kind == T_TRACK ? (i64)e_plo + o1 : (i64)e_plo + 1;
            if (e_kind != T_ZERO) okc = xa >= x_lo && xb <= x_lo + wlen && xa >= 0 && xb <= tlen;
        }
        if (__builtin_amdgcn_ballot_w64(!okc) != 0) fast = false;
    }
    if (!fast) {
        realign_chunk_general(kernarg, (TrackMirrorLds)&mirror[wave], (PaintWinLds)&W, k, chunk, n_chunks);
        return;
    }
#ifdef GVL_DIAG
    if (A.stamps && lane == 0 && !tl_on) { atomicAdd((unsigned long long *)&A.stamps[8], 1ull); atomicAdd((unsigned long long *)&A.stamps[15], 1ull); }
#else
    if (A.stamps && lane == 0) { atomicAdd((unsigned long long *)&A.stamps[8], 1ull); atomicAdd((unsigned long long *)&A.stamps[15], 1ull); }
#endif
    // ---- emit
    const bool rc = ((rc_word >> (8 * (int)(rc_addr & 3ull))) & 0xFF) != 0;
    float *const out_row = A.out + row_base;
    const int xl = (int)x_lo;
    auto in_win = [&](const int r) -> float {
        const u32 wd = W.bm[r >> 5];
        return W.bv[(int)W.pre[r >> 5] + __builtin_popcount(wd & (0xFFFFFFFFu >> (31 - (r & 31))))];
    };
    auto win4 = [&](const int r, float (&v)[4]) {
        const int bp = r & 31, wi = r >> 5;
        const u64 w = ((u64)W.bm[wi + 1] << 32) | W.bm[wi];
        const int c0 = (int)W.pre[wi] + __builtin_popcountll(w & (~0ull >> (63 - bp)));
        const u32 m = (u32)(w >> (bp + 1));
        v[0] = W.bv[c0];
#pragma unroll
        for (int g = 1; g < 4; ++g) v[g] = W.bv[c0 + __builtin_popcount(m & ((1u << g) - 1u))];
    };
    int p0 = lo_clip;
    while (p0 < hi_clip) {
        int li = __builtin_popcountll(__builtin_amdgcn_ballot_w64(ev && e_out <= p0)) - 1;
        li = li < 0 ? 0 : li;
        {
            const int kd = rdl(e_kind, li), plo = rdl(e_plo, li);
            int nx = li + 1 < nseg ? rdl(e_out, li + 1) : hi_clip;
            nx = nx < hi_clip ? nx : hi_clip;
            const int n2 = (nx - p0) / (2 * TRIP);
            if (kd == T_TRACK && n2 > 0) {
                // a run's double trips: position and output pointer advance by a constant; two groups of four per lane, one contiguous KB
                // per store instruction
                int r = plo + p0 + GROUP * lane - xl;
                float *o = rc ? out_row + (L - GROUP - (p0 + GROUP * lane)) : out_row + (p0 + GROUP * lane);
                const int ostep = rc ? -2 * TRIP : 2 * TRIP;
#pragma unroll 1
                for (int i = 0; i < n2; ++i) {
                    float q1[GROUP], q2[GROUP];
                    win4(r, q1); win4(r + TRIP, q2);
                    if (!rc) {
                        store_f32x4(o, q1[0], q1[1], q1[2], q1[3]);
                        store_f32x4(o + TRIP, q2[0], q2[1], q2[2], q2[3]);
                    } else {
                        store_f32x4(o, q1[3], q1[2], q1[1], q1[0]);
                        store_f32x4(o - TRIP, q2[3], q2[2], q2[1], q2[0]);
                    }
                    r += 2 * TRIP; o += ostep;
                }
                p0 += n2 * (2 * TRIP);
                continue;
            }
        }
        // one trip, entry by entry (each wave-uniform: kind, delta and range are scalars; a lane takes the positions of its group that lie inside)
        const int p = p0 + GROUP * lane;
        const int trip_end = (hi_clip - p0 > TRIP) ? p0 + TRIP : hi_clip;
        float v4[GROUP] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (;;) {
            const int st_e = rdl(e_out, li), kd = rdl(e_kind, li), plo = rdl(e_plo, li);
            int nx = li + 1 < nseg ? rdl(e_out, li + 1) : hi_clip;
            nx = nx < trip_end ? nx : trip_end;
            if (kd == T_TRACK) {
                if (p >= st_e && p + GROUP <= nx) {
                    win4(plo + p - xl, v4);
                } else {
#pragma unroll
                    for (int g = 0; g < GROUP; ++g)
                        if (p + g >= st_e && p + g < nx) v4[g] = in_win(plo + p + g - xl);
                }
            } else if (kd == T_REPEAT) {
                const float v = in_win(plo - xl);                            // (one position for the whole entry)
#pragma unroll
                for (int g = 0; g < GROUP; ++g)
                    if (p + g >= st_e && p + g < nx) v4[g] = v;
            }                                                                // (T_ZERO: stays 0)
            if (nx >= trip_end || li + 1 >= nseg) break;
            ++li;
        }
        if (p + GROUP <= hi_clip) {
            if (!rc) store_f32x4(out_row + p, v4[0], v4[1], v4[2], v4[3]);
            else store_f32x4(out_row + (L - GROUP - p), v4[3], v4[2], v4[1], v4[0]);
        } else {
#pragma unroll
            for (int i = 0; i < GROUP; ++i)
                if (p + i < hi_clip) out_row[rc ? (L - 1 - (p + i)) : (p + i)] = v4[i];
        }
        p0 += TRIP;
    }
    PAINT_STAMP(5);
