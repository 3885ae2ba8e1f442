// gvl_recon_body.inc -- the all-purpose reconstruct body (recon_body: scan-free / packed / per-wave-scan plans, the scalar walk)
// that reconstruct_kernel instantiates 12 ways and the lean kernels call in SOLO mode for the rows they do not take.
// Included inside the including file's anonymous namespace, behind gvl_dev.inc.

// ---------------------------------------------------------------------------------
// Scalar path: ONE wave replays the reference's walk on the scalar unit and streams its
// (row, chunk).  Handles everything (any number of variants / segments, via flush +
// compaction of the 64-entry lane tables).  It is the fallback of the planned path below
// for rows the cooperative planner does not take (more than CAP_V variants, table
// overflow) -- it costs ~10x more issue slots per row, so it is not the default.
// ---------------------------------------------------------------------------------
template <int OH, bool HAPS, bool ANNOT>
__device__ __forceinline__ void recon_wave_scalar(const ReconArgs &A, const Luts &luts, SegMirror &M,
                                                   Stage<ANNOT> &G, const i64 k, const int chunk,
                                                   const int lane) {
    const i64 query = A.ploidy_shift >= 0 ? (k >> A.ploidy_shift) : (i64)((u32)k / (u32)A.ploidy);

    // ---- row parameters (level-1 loads; wave-uniform) -------------------------
    const int *reg = A.regions + query * A.regions_stride;
    const i64 c_idx = rfl(reg[0]);
    const i64 ref_start = rfl(reg[1]);
    i64 shift = 0, o_idx = 0;
    bool ref_zero_fill = false;
    if (!A.ref_only) {
        shift = rfl(A.shifts[k]);
        o_idx = rfl64(A.geno_offset_idx[k]);
    } else {
        ref_zero_fill = ref_start >= (i64)rfl(reg[2]);   // reference/mod.rs:16-18
    }
    const bool rc = A.to_rc ? (rfl((int)A.to_rc[k]) != 0) : false;
    i64 row_base; int L;
    if (A.out_offsets) {
        row_base = rfl64(A.out_offsets[k << A.oo_shift]);
        L = (int)(rfl64(A.out_offsets[(k << A.oo_shift) + 1]) - row_base);
    } else {
        row_base = k * A.fixed_len;
        L = (int)A.fixed_len;
    }
    if (A.out_offsets_w && chunk == 0 && lane == 0) {
        A.out_offsets_w[k] = row_base;
        if (k == A.n_rows - 1) A.out_offsets_w[k + 1] = row_base + L;
    }
    const int lo_clip = chunk * A.chunk_len;
    if (lo_clip >= L) return;
    const int hi_clip = (L - lo_clip > A.chunk_len) ? lo_clip + A.chunk_len : L;

    // ---- level-2 loads ---------------------------------------------------------
    const i64 c_s = rfl64(A.ref_offsets[c_idx]);
    const i64 R = rfl64(A.ref_offsets[c_idx + 1]) - c_s;
    const bool has_keep = A.keep && A.keep_offsets;
    i64 o_s = 0, keep_off = 0;
    int n_var = 0;
    if (!A.ref_only) {
        o_s = rfl64(A.go_starts[o_idx]);
        const i64 nv = rfl64(A.go_stops[o_idx]) - o_s;
        n_var = nv < 0 ? 0 : (nv > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)nv);
        if (A.dbg & GVL_ABL(DBG_ABL_NO_VARIANTS)) n_var = 0;
        if (has_keep) keep_off = rfl64(A.keep_offsets[k]);
    }

    // ---- segment / patch tables (lane s holds entry s) ------------------------
    int s_out = 0; u32 s_lo = 0, s_hi = 0; int s_a = 0, s_b = 0;
    int p_out = 0, p_val = 0, p_id = 0;
    int nseg = 0, npatch = 0;
    u32 last_kind = 0xFFu; i64 last_delta = 0;

    // Append a segment [o_start, o_start+len) of `kind` whose byte at output position p
    // is source[delta + p].  Output coordinates are ints (< 2^31); a reference run that
    // continues the previous one (same delta) is merged, which is what makes SNPs free.
    auto push = [&](u32 kind, int o_start, int len, i64 src, int id, int vpos) {
        if (len <= 0 || o_start + len <= lo_clip || o_start >= hi_clip) return;
        const i64 delta = src - o_start;
        if (kind == K_REF && last_kind == K_REF && delta == last_delta) return;
        const u64 enc = (u64)(delta + DELTA_BIAS) | ((u64)kind << 62);
        if (lane == nseg) {
            s_out = o_start; s_lo = (u32)enc; s_hi = (u32)(enc >> 32);
            if (ANNOT) { s_a = id; s_b = vpos; }
        }
        last_kind = kind; last_delta = delta; ++nseg;
    };

    // ---- walk state: reconstruct/mod.rs:61-83 -----------------------------------
    i64 ref_idx = ref_start, shifted = 0;
    int out_idx = 0;
    if (ref_idx < 0) {
        const i64 raw = -ref_idx;
        shifted = imin(shift, raw);
        // a pad longer than the row is clamped: the row is then all pad either way
        const int n = (int)imin(raw - shifted, (i64)L);
        push(K_PAD_LEAD, 0, n, 0, -1, -1);
        out_idx = n;
        ref_idx = 0;
    }

    // variant record registers for the current trip of 64 variants
    int r_pos = 0, r_ilen = 0, r_alen = 0, r_inl = 0, r_vi = 0, r_a0lo = 0, r_a0hi = 0, r_keep = 1;
    int vi = 0;          // next variant of the row
    int vb = -WAVE;      // base of the loaded trip
    bool walk_done = false;
    int emit_pos = lo_clip;

    const u32 padb = A.pad & 0xFFu;
    // RC is folded into the store: forward position p lands at L-4-p (group) with the
    // group's 4 bytes reversed (one v_perm with a uniform selector) and complemented
    // (second LUT).  `lane_off` is the lane's share of the store offset, in bases.
    const u32 rc_sel = rc ? 0x00010203u : 0x03020100u;
    const u32 *oh_t = rc ? luts.oh_rc : luts.oh;
    const int lane_pos = rc ? -GROUP * lane : GROUP * lane;
    u8 *hap_row = HAPS ? A.haps + row_base : nullptr;
    u8 *oh_row = OH != OH_NONE ? A.onehot + 4 * row_base : nullptr;
    int *av_row = (ANNOT && A.av) ? A.av + row_base : nullptr;
    int *ap_row = (ANNOT && A.ap) ? A.ap + row_base : nullptr;

    for (;;) {
        // =================== fill: replay the reference walk =====================
        while (!walk_done && nseg <= SEG_FLUSH && npatch <= PATCH_FLUSH) {
            bool stop = (vi >= n_var) || (out_idx >= hi_clip);
            if (!stop) {
                if (vi - vb >= WAVE) {
                    // gather the next 64 variant records (levels 3 and 4)
                    vb = vi;
                    const int j = vb + lane;
                    const bool valid = j < n_var;
                    int v = valid ? A.geno_v_idxs[o_s + j] : 0;
                    v = v < 0 ? 0 : ((i64)v >= A.n_variants ? (int)(A.n_variants - 1) : v);
                    r_vi = v;
                    if (valid) {
                        const i32x4 rec = *reinterpret_cast<const i32x4 *>(A.vrec + v);
                        const i64 a0 = A.alt_offsets[v];
                        r_pos = rec.x; r_ilen = rec.y; r_alen = rec.z; r_inl = rec.w;
                        r_a0lo = (int)(u32)(u64)a0; r_a0hi = (int)(u32)((u64)a0 >> 32);
                        r_keep = has_keep ? (int)A.keep[keep_off + j] : 1;
                    }
                }
                const int i = vi - vb;
                ++vi;
                // --- one step of reconstruct/mod.rs:85-198 ---
                if (has_keep && rdl(r_keep, i) == 0) continue;           // :86-90
                const i64 pos = rdl(r_pos, i);
                const int d = rdl(r_ilen, i);
                const int alen = rdl(r_alen, i);
                const i64 v_end = pos - (d < 0 ? (i64)d : 0) + 1;         // :96
                if (pos < ref_idx) {
                    // :99-102 DEL spanning the window start (only possible while pos < ref_start
                    // <= ref_idx), else :108-110 first ALT wins
                    if (pos < ref_start && d < 0 && v_end >= ref_start) ref_idx = v_end;
                    continue;
                }
                i64 skip = 0;
                if (shifted < shift) {                                    // :115-146
                    const i64 dist = pos - ref_idx;
                    if (shifted + dist + alen < shift) continue;
                    if (shifted + dist >= shift) {
                        ref_idx += shift - shifted;
                        shifted = shift;
                    } else {
                        skip = shift - shifted - dist;
                        shifted = shift;
                        if (skip == alen) { ref_idx = v_end; continue; }
                        ref_idx = pos;
                    }
                }
                const i64 n64 = pos - ref_idx;
                if (n64 >= (i64)(L - out_idx)) {                          // :154-158 (">=")
                    stop = true;
                } else {
                    const int n = (int)n64;
                    const int id = rdl(r_vi, i);
                    if (d == 0 && alen == 1) {
                        // pure SNP (skip == 0 here): the reference run continues through the
                        // variant's own base and one output byte is patched
                        push(K_REF, out_idx, n + 1, c_s + ref_idx, -1, -1);
                        out_idx += n;
                        if (out_idx >= lo_clip && out_idx < hi_clip) {
                            if (lane == npatch) { p_out = out_idx; p_val = rdl(r_inl, i) & 0xFF; if (ANNOT) p_id = id; }
                            ++npatch;
                        }
                        out_idx += 1;
                    } else {
                        push(K_REF, out_idx, n, c_s + ref_idx, -1, -1);
                        out_idx += n;
                        const i64 al = (i64)alen - skip;
                        const int w = (int)imin(al, (i64)(L - out_idx));  // :178
                        push(K_ALLELE, out_idx, w, rdl64(r_a0lo, r_a0hi, i) + skip, id, (int)pos);
                        out_idx += w;
                    }
                    ref_idx = v_end;                                      // :193
                    if (out_idx >= L) stop = true;                        // :195-197
                }
            }
            if (stop) {
                // residual shift + tail: reconstruct/mod.rs:200-255
                if (shifted < shift) ref_idx = imin(ref_idx + (shift - shifted), R);
                const int u = L - out_idx;
                if (u > 0) {
                    const i64 avail = R - ref_idx;
                    const int w = (int)imin((i64)u, avail);
                    int end = out_idx;
                    if (w > 0) { push(K_REF, out_idx, w, c_s + ref_idx, -1, -1); end += w; }
                    if (end < L) push(K_PAD_TRAIL, end, L - end, 0, -1, -1);
                }
                out_idx = out_idx > L ? out_idx : L;
                walk_done = true;
            }
        }

        // =================== emit [emit_pos, limit) ===============================
        // One trip = 256 bases, 4 per lane.  A trip that lies inside ONE reference run
        // (the common case) is "uniform": every lane loads its 4 bytes from a scalar
        // base.  Other trips take the general path: per-lane segment lookup through the
        // LDS mirror; lanes on a boundary / in an allele / pad / row end assemble their
        // 4 bytes one by one.  Then: SNP patches, reverse-complement, one-hot LUT, store.
        const int cov = out_idx < lo_clip ? lo_clip : (out_idx > hi_clip ? hi_clip : out_idx);
        const int limit = walk_done ? hi_clip : (cov & ~3);
        int sc = -1, pc = 0;
        int c_next = emit_pos;      // start of segment sc+1 (or cov)
        bool c_ok = false;          // segment sc is a reference run that stays inside `ref`
        const u8 *c_base = A.ref;   // A.ref + delta of segment sc
        int c_apb = 0;              // annotation: contig coordinate of output position 0
        int np_pos = npatch > 0 ? rdl(p_out, 0) : 0x7FFFFFFF;
        bool mirror_valid = false;
        for (int p0 = emit_pos; p0 < limit; p0 += TRIP) {
            const int t_end = (limit - p0 > TRIP) ? p0 + TRIP : limit;
            while (c_next <= p0) {      // advance to the segment that holds p0
                ++sc;
                const u32 hi = (u32)rdl((int)s_hi, sc);
                const i64 dl = seg_delta((u32)rdl((int)s_lo, sc), hi);
                const int c_start = rdl(s_out, sc);
                c_next = sc + 1 < nseg ? rdl(s_out, sc + 1) : cov;
                const int e = c_next < limit ? c_next : limit;
                c_ok = (hi >> 30) == K_REF && dl + (c_start > emit_pos ? c_start : emit_pos) >= 0 &&
                       dl + e <= A.ref_len && !ref_zero_fill;
                c_base = A.ref + dl;
                if (ANNOT) c_apb = (int)(dl - c_s);
            }
            const int p = p0 + GROUP * lane;
            const bool act = p < limit;
            const bool full = p + GROUP <= limit;
            u32 wv = 0;
            int av4[GROUP], ap4[GROUP];
            if (c_ok && c_next >= t_end && ((t_end - p0) & 3) == 0) {
                // ---- uniform trip -------------------------------------------------
                if (act && !(A.dbg & GVL_ABL(DBG_ABL_NO_LOADS))) wv = load_u32_unaligned(c_base + p0 + (u32)(GROUP * lane));
                if (ANNOT) {
#pragma unroll
                    for (int i = 0; i < GROUP; ++i) { av4[i] = -1; ap4[i] = c_apb + p + i; }
                }
            } else {
                // ---- general trip -------------------------------------------------
                if (!mirror_valid) {
                    M.out[lane] = s_out; M.lo[lane] = s_lo; M.hi[lane] = s_hi;
                    if (ANNOT) { M.a[lane] = s_a; M.b[lane] = s_b; }
                    mirror_valid = true;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
                if (act) {
                    // largest li with M.out[li] <= p (binary search; nseg <= 64)
                    int li = 0;
#pragma unroll
                    for (int step = 32; step > 0; step >>= 1) {
                        const int t = li + step;
                        if (t < nseg && M.out[t] <= p) li = t;
                    }
                    const u32 l0 = M.lo[li], h0 = M.hi[li];
                    const int nx = li + 1 < nseg ? M.out[li + 1] : cov;
                    const i64 src = seg_delta(l0, h0) + p;
                    if ((h0 >> 30) == K_REF && p + GROUP <= nx && full && src >= 0 &&
                        src + GROUP <= A.ref_len && !ref_zero_fill) {
                        wv = load_u32_unaligned(A.ref + src);
                        if (ANNOT) {
#pragma unroll
                            for (int i = 0; i < GROUP; ++i) { av4[i] = -1; ap4[i] = (int)(src - c_s) + i; }
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < GROUP; ++i) {
                            const int pp = p + i;
                            u32 b = 0; int a_v = -1, a_p = -1;
                            if (pp < limit) {
                                while (li + 1 < nseg && M.out[li + 1] <= pp) ++li;
                                const u32 l2 = M.lo[li], h2 = M.hi[li];
                                const u32 k2 = h2 >> 30;
                                const i64 s2 = seg_delta(l2, h2) + pp;
                                if (ref_zero_fill) {
                                    b = 0;
                                } else if (k2 == K_REF) {
                                    b = (s2 >= 0 && s2 < A.ref_len) ? (u32)A.ref[s2] : padb;
                                    a_p = (int)(s2 - c_s);
                                } else if (k2 == K_ALLELE) {
                                    b = (s2 >= 0 && s2 < A.alt_len) ? (u32)A.alt_alleles[s2] : padb;
                                    if (ANNOT) { a_v = M.a[li]; a_p = M.b[li]; }
                                } else {
                                    b = padb;
                                    a_p = (k2 == K_PAD_LEAD) ? -1 : 2147483647;
                                }
                            }
                            wv |= b << (8 * i);
                            if (ANNOT) { av4[i] = a_v; ap4[i] = a_p; }
                        }
                    }
                }
            }
            // ---- SNP patches that land in this trip (sorted; scalar cursor) ----------
            while (np_pos < t_end) {
                const u32 dd = (u32)(np_pos - p);
                if (dd < (u32)GROUP) {
                    const u32 sh = dd * 8;
                    wv = (wv & ~(0xFFu << sh)) | ((u32)rdl(p_val, pc) << sh);
                }
                if (ANNOT) {
                    const int pid = rdl(p_id, pc);
#pragma unroll
                    for (int i = 0; i < GROUP; ++i) if (dd == (u32)i) av4[i] = pid;
                }
                ++pc;
                np_pos = pc < npatch ? rdl(p_out, pc) : 0x7FFFFFFF;
            }
            // ---- stores ------------------------------------------------------------------
            if (full && !(A.dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
                // forward: jo = p; RC: jo = L - 4 - p.  In both cases jo = jo0 + lane_pos.
                const int jo = (rc ? L - GROUP - p0 : p0) + lane_pos;
                const u32 ww = __builtin_amdgcn_perm(0u, wv, rc_sel);
                const u32 b0_ = ww & 0xFF, b1_ = (ww >> 8) & 0xFF, b2_ = (ww >> 16) & 0xFF, b3_ = ww >> 24;
                if (OH == OH_LC) {
                    u32x4_a4 o = {oh_t[b0_], oh_t[b1_], oh_t[b2_], oh_t[b3_]};
                    store_oh16(oh_row + 4 * (i64)jo, o);
                } else if (OH == OH_CL) {
                    // channel-major (rows, 4, L): plane a holds byte a of each one-hot dword
                    const u32 d0 = oh_t[b0_], d1 = oh_t[b1_], d2 = oh_t[b2_], d3 = oh_t[b3_];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const u32 sh = 8 * a;
                        const u32 v = ((d0 >> sh) & 0xFF) | (((d1 >> sh) & 0xFF) << 8) |
                                      (((d2 >> sh) & 0xFF) << 16) | (((d3 >> sh) & 0xFF) << 24);
                        store_u32_unaligned(oh_row + (i64)a * L + jo, v);
                    }
                }
                if (HAPS) {
                    u32 hv = ww;
                    if (rc) hv = (u32)luts.comp[b0_] | ((u32)luts.comp[b1_] << 8) | ((u32)luts.comp[b2_] << 16) | ((u32)luts.comp[b3_] << 24);
                    store_u32_unaligned(hap_row + jo, hv);
                }
                if (ANNOT) {
                    if (av_row) {
                        i32x4_a4 o = rc ? i32x4_a4{av4[3], av4[2], av4[1], av4[0]} : i32x4_a4{av4[0], av4[1], av4[2], av4[3]};
                        store_i32x4(av_row + jo, o.x, o.y, o.z, o.w);
                    }
                    if (ap_row) {
                        i32x4_a4 o = rc ? i32x4_a4{ap4[3], ap4[2], ap4[1], ap4[0]} : i32x4_a4{ap4[0], ap4[1], ap4[2], ap4[3]};
                        store_i32x4(ap_row + jo, o.x, o.y, o.z, o.w);
                    }
                }
            }
            if (limit & 3) {
                // the partial group at the row end (L % 4 != 0): the owning lane parks its
                // patched bytes; lanes 0..(L&3)-1 then store one base each
                const int p_last = limit & ~3;
                if (p_last >= p0 && p_last < p0 + TRIP) {
                    if (act && !full) {
                        G.w[0] = wv;
                        if (ANNOT) {
#pragma unroll
                            for (int i = 0; i < GROUP; ++i) { G.av[i][0] = av4[i]; G.ap[i][0] = ap4[i]; }
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (lane < (limit & 3)) {
                        const int pp = p_last + lane;
                        const u32 b = (G.w[0] >> (8 * lane)) & 0xFF;
                        const i64 jo = rc ? (i64)(L - 1 - pp) : (i64)pp;
                        if (OH != OH_NONE) {
                            const u32 d = oh_t[b];
                            if (OH == OH_LC) {
                                __builtin_memcpy(oh_row + 4 * jo, &d, 4);
                            } else {
#pragma unroll
                                for (int a = 0; a < 4; ++a) oh_row[(i64)a * L + jo] = (u8)((d >> (8 * a)) & 0xFF);
                            }
                        }
                        if (HAPS) hap_row[jo] = (u8)(rc ? luts.comp[b] : b);
                        if (ANNOT) {
                            if (av_row) av_row[jo] = G.av[lane][0];
                            if (ap_row) ap_row[jo] = G.ap[lane][0];
                        }
                    }
                }
            }
        }
        emit_pos = limit;
        if (walk_done || emit_pos >= hi_clip) break;

        // =================== compact: drop what has been emitted ==================
        {
            int cnt = 0;
            for (int s = 0; s < nseg; ++s) cnt += (rdl(s_out, s) <= emit_pos) ? 1 : 0;
            const int s0 = cnt > 0 ? cnt - 1 : 0;
            if (s0 > 0) {
                const int srcl = lane + s0 < SEG_CAP ? lane + s0 : SEG_CAP - 1;
                s_out = bperm(srcl, s_out);
                s_lo = (u32)bperm(srcl, (int)s_lo);
                s_hi = (u32)bperm(srcl, (int)s_hi);
                if (ANNOT) { s_a = bperm(srcl, s_a); s_b = bperm(srcl, s_b); }
                nseg -= s0;
            }
            int pcnt = 0;
            for (int s = 0; s < npatch; ++s) pcnt += (rdl(p_out, s) < emit_pos) ? 1 : 0;
            if (pcnt > 0) {
                const int srcl = lane + pcnt < WAVE ? lane + pcnt : WAVE - 1;
                p_out = bperm(srcl, p_out);
                p_val = bperm(srcl, p_val);
                if (ANNOT) p_id = bperm(srcl, p_id);
                npatch -= pcnt;
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// Planned path.  A workgroup = 8 waves = 8 rows of one chunk index; wave w owns row w.
//   P1  lanes 0..7 of wave 0 load the 8 rows' parameters (one lane per row), one barrier
//   P2  the row's variant records, lane j = variant j; rows with <= 8 variants classify
//       themselves: fast (SNPs only: the scan-free plan in reconstruct_kernel) or slow
//       (planned together by the first slow wave: packed_plan); the others run P3 per wave
//   P3  the reference's sequential walk, restated as wave-wide scans:
//         * shift: the lead pad absorbs it first; while it is open ref_idx does not move, so
//           the variants in front of the one that completes it are dropped and that one is
//           kept / cut at the front / consumed (a ballot + ctz)
//         * "first ALT wins": variant i is applied iff pos_i >= max(ref_idx0, v_end of every
//           applied variant before it) -- an exclusive prefix-max, iterated to its (unique)
//           fixed point when deletions knock out later variants
//         * output offsets of the applied variants: exclusive prefix-sum of
//           (reference run + allele length) -- the indel shift
//         * the loop's ">= L" break: applied = prefix of lanes whose allele starts before L
//         * segment table: one REF run + one ALLELE entry per applied indel (SNPs do not
//           split a run, they become patches), scattered to LDS at prefix-count slots
//   P3b lanes 0..7, one per trip, turn the table into trip descriptors: "uniform" trips
//       (inside ONE reference run) carry the source offset; plus the trip's patch slice
//   P4  the wave streams its row from the descriptors, all reference loads issued first
// Rows the scans do not take (> 64 variants, table overflow, coordinates >= 2^30, negative
// shift, no fixed point in 4 rounds) run recon_wave_scalar instead.
// ---------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------
// Packed plan: ONE wave plans all 8 rows of the workgroup at once, lane = (row r = lane / 8,
// variant j = lane % 8), for rows with at most 8 variants (99.7 % of cfg2 / cfg3 rows).  The
// same restatement of the walk as the per-wave P3 below, with the scans confined to groups of 8
// lanes; then P3b with lane = (row, trip).  It exists because the plan is a dependent
// instruction chain: eight waves each running it for one row take eight times the issue slots
// (and a row with an indel, whose plan is the longest, ends the launch), one wave running it
// for eight rows takes the same chain once.
// ---------------------------------------------------------------------------------
template <bool ANNOT>
__device__ __forceinline__ void packed_plan(const ReconArgs &A, const RowIn *rin, RowPlan<ANNOT> *plan, TripDesc *desc,
                                            RowMeta *meta, const i32x4 *lrec, const int lane, const int lo_clip, const bool has_keep) {
    const int r = lane >> 3, j = lane & 7, seg_base = lane & ~7;
    const RowIn &ri = rin[r];
    RowPlan<ANNOT> &pl = plan[r];
    const int rflags = ri.flags;
    const bool elig = (rflags & 9) == 8 && meta[r].slow != 0;
    const int L = ri.L;
    const i64 c_s = ri.c_s, R = ri.R;
    const int hi_clip = (L - lo_clip > A.chunk_len) ? lo_clip + A.chunk_len : L;
    const int n_var = ri.n_var;
    const i64 o_s = ri.o_s;
    const i64 rs64 = ri.ref_start;
    bool ok = rs64 > -(1 << 30) && rs64 < (1 << 30);
    const int ref_start = ok ? (int)rs64 : 0;
    const int shift_i = (int)ri.shift;                 // [0, 2^30): checked in P1
    auto seg_byte = [&](u64 m) -> u32 { return (u32)(m >> seg_base) & 0xFFu; };

    // ---- P2: records ----------------------------------------------------------------
    int pos = 0, d = 0, alen = 0, inl = 0, vi = 0; i64 a0 = 0;
    const bool ell = (rflags & 16) != 0;               // slot-major records: 8 entries at srec[slot * 8]
    bool valid = elig && j < n_var;
    if (valid) {
        if (ell) {
            const i32x4 rec = lrec[lane];                  // parked in LDS by P1: lane = row x 8 + entry
            const u32 e = (u32)rec.z;
            valid = e != GVL_SREC_EMPTY;
            pos = rec.x; d = rec.y; alen = (int)(e >> 8); inl = (int)(e & 0xFF); vi = 0;
            a0 = (i64)(u32)rec.w;                          // no alt_offsets hop
        } else if (A.grec) {
            const i32x4 rec = *reinterpret_cast<const i32x4 *>(A.grec + (o_s + j));
            pos = rec.x; d = rec.y; alen = (int)((u32)rec.z >> 8); inl = rec.z & 0xFF; vi = rec.w;
            if (!(d == 0 && alen == 1)) a0 = A.alt_offsets[vi];
        } else {
            int v = A.geno_v_idxs[o_s + j];
            v = v < 0 ? 0 : ((i64)v >= A.n_variants ? (int)(A.n_variants - 1) : v);
            const i32x4 rec = *reinterpret_cast<const i32x4 *>(A.vrec + v);
            a0 = A.alt_offsets[v];
            pos = rec.x; d = rec.y; alen = rec.z; inl = rec.w; vi = v;
        }
        if (valid && has_keep) valid = A.keep[ri.keep_off + j] != 0;
    }
    const bool weird = valid && (pos < 0 || pos >= (1 << 30) || d <= -(1 << 30) || d >= (1 << 30) || alen < 0 ||
                                 alen >= ((ell || A.grec) ? 0xFFFFFF : (1 << 30)));
    ok = ok && seg_byte(__builtin_amdgcn_ballot_w64(weird)) == 0;
    if (!ok) valid = false;

    // ---- P3 ---------------------------------------------------------------------------
    const int raw = ref_start < 0 ? -ref_start : 0;
    const int shifted0 = shift_i < raw ? shift_i : raw;
    const int n_lead = (raw - shifted0 < L) ? raw - shifted0 : L;
    int rem = shift_i - shifted0;
    int ref_idx0 = ref_start < 0 ? 0 : ref_start;
    const int lead_kept = (n_lead > 0 && n_lead > lo_clip && 0 < hi_clip) ? 1 : 0;
    const int E = pos - (d < 0 ? d : 0) + 1;
    const bool is_snp = d == 0 && alen == 1;
    {   // DEL spanning the window start: the last one in order sets ref_idx
        const u32 b = seg_byte(__builtin_amdgcn_ballot_w64(valid && pos < ref_start && d < 0 && E >= ref_start));
        const int src = seg_base + (b ? 31 - __builtin_clz(b) : 0);
        const int e_src = bperm(src, E);
        if (b) ref_idx0 = e_src;
    }
    bool cand = valid && pos >= ref_start;
    int a_skip = 0;     // a0 (a second dependent load for indel lanes) is first touched at the very end
    {   // shift consumption
        const int base = ref_idx0;
        const u32 b = seg_byte(__builtin_amdgcn_ballot_w64(rem > 0 && cand && pos >= base && (pos - base) + alen >= rem));
        const int f = b ? __builtin_ctz(b) : 0;
        const int fl = seg_base + f;
        const int pos_f = bperm(fl, pos), alen_f = bperm(fl, alen), E_f = bperm(fl, E);
        if (rem > 0) {
            if (b == 0) {
                cand = false;
            } else {
                const int dist = pos_f - base;
                if (dist >= rem) {
                    ref_idx0 = base + rem;
                    cand = cand && j >= f;
                } else {
                    const int skip = rem - dist;
                    if (skip == alen_f) {
                        ref_idx0 = E_f;
                        cand = cand && j > f;
                    } else {
                        ref_idx0 = pos_f;
                        cand = cand && j >= f;
                        if (j == f) { alen -= skip; a_skip = skip; }
                    }
                }
                rem = 0;
            }
        }
    }
    const int pm_carry = ref_idx0;
    // first ALT wins: fixed point, all rows at once
    bool inB = cand;
    int PM = 0;
    {
        u64 mB = __builtin_amdgcn_ballot_w64(inB);
        bool stable = false;
#pragma unroll 1
        for (int it = 0; it < 4 && !stable; ++it) {
            PM = seg8_scan_exclusive<OpMaxU>(inB ? E : 0, j);
            PM = PM > pm_carry ? PM : pm_carry;
            inB = cand && pos >= PM;
            const u64 m2 = __builtin_amdgcn_ballot_w64(inB);
            stable = m2 == mB;
            if (it == 3) ok = ok && seg_byte(m2) == seg_byte(mB);
            mB = m2;
        }
    }
    const int n_i = inB ? pos - PM : 0;
    const int S_i = inB ? OpSat::f(n_i, alen) : 0;
    const int X = seg8_scan_exclusive<OpSat>(S_i, j);
    const int allele_out = OpSat::f(OpSat::f(n_lead, X), n_i);
    const bool applied = inB && allele_out < L;
    const int w_i = applied ? ((alen < L - allele_out) ? alen : L - allele_out) : 0;
    const bool nonsnp = applied && !is_snp;
    const bool snp = applied && is_snp;
    const u32 b_app = seg_byte(__builtin_amdgcn_ballot_w64(applied));
    const bool any_applied = b_app != 0;
    int ref_idx_end = ref_idx0, out_idx_end = n_lead;
    {
        const int last = seg_base + (b_app ? 31 - __builtin_clz(b_app) : 0);
        const int e_l = bperm(last, E), o_l = bperm(last, allele_out + w_i);
        if (b_app) { ref_idx_end = e_l; out_idx_end = o_l; }
    }
    const int prevNS = seg8_scan_exclusive<OpMaxI>(nonsnp ? j : -1, j);
    const int pidx = seg_base + (prevNS < 0 ? 0 : prevNS);
    const int p_end = bperm(pidx, allele_out + alen);
    const int p_E = bperm(pidx, E);
    const int run_start = prevNS < 0 ? n_lead : p_end;
    const i64 run_src = c_s + (prevNS < 0 ? ref_idx0 : p_E);
    const bool e_ref = nonsnp && allele_out > run_start && allele_out > lo_clip && run_start < hi_clip;
    const bool e_all = nonsnp && w_i > 0 && allele_out + w_i > lo_clip && allele_out < hi_clip;
    const int slot0 = lead_kept + seg8_scan_exclusive<OpAdd>((e_ref ? 1 : 0) + (e_all ? 1 : 0), j);
    const u32 b_ns = seg_byte(__builtin_amdgcn_ballot_w64(nonsnp));
    const u32 b_snp = seg_byte(__builtin_amdgcn_ballot_w64(snp && allele_out >= lo_clip && allele_out < hi_clip));
    const int n_ent = lead_kept + __builtin_popcount(seg_byte(__builtin_amdgcn_ballot_w64(e_ref))) +
                      __builtin_popcount(seg_byte(__builtin_amdgcn_ballot_w64(e_all)));
    const int npatch = __builtin_popcount(b_snp);
    auto put = [&](int q, u32 kind, int o_start, i64 delta, int id, int vpos) {
        const u64 e = (u64)(delta + DELTA_BIAS) | ((u64)kind << 62);
        pl.s_out[q] = o_start; pl.s_lo[q] = (u32)e; pl.s_hi[q] = (u32)(e >> 32);
        if (ANNOT) { pl.s_a[q] = id; pl.s_b[q] = vpos; }
    };
    if (ok && elig) {
        int q = slot0;
        if (e_ref) { put(q, K_REF, run_start, run_src - run_start, -1, -1); ++q; }
        if (e_all) put(q, K_ALLELE, allele_out, a0 + a_skip - allele_out, vi, pos);
        if ((b_snp >> j) & 1u) {
            const int ps = __builtin_popcount(b_snp & ((1u << j) - 1u));
            pl.p_out[ps] = allele_out; pl.p_val[ps] = inl & 0xFF;
            if (ANNOT) pl.p_id[ps] = vi;
        }
    }
    // last applied indel of the row -> start of the tail run
    int ns_end = 0, ns_E = 0;
    {
        const int ln = seg_base + (b_ns ? 31 - __builtin_clz(b_ns) : 0);
        ns_end = bperm(ln, allele_out + alen);
        ns_E = bperm(ln, E);
    }
    const bool have_ns = b_ns != 0;
    if (rem > 0) ref_idx_end = (int)imin((i64)ref_idx0 + rem, R);
    const int t_start = have_ns ? ns_end : n_lead;
    const i64 t_src = c_s + (have_ns ? ns_E : ((rem > 0 && !any_applied) ? ref_idx_end : ref_idx0));
    int t_end = out_idx_end;
    {
        const int u = L - out_idx_end;
        if (u > 0) {
            const int w = (int)imin((i64)u, R - ref_idx_end);
            if (w > 0) t_end = out_idx_end + w;
        }
    }
    const bool tail_pad = t_end < L && L > lo_clip && t_end < hi_clip;
    const bool tail_ref = t_end > t_start && t_end > lo_clip && t_start < hi_clip;
    const int nseg = n_ent + (tail_ref ? 1 : 0) + (tail_pad ? 1 : 0);
    if (ok && elig) {
        if (j == 0) {
            if (lead_kept) put(0, K_PAD_LEAD, 0, 0, -1, -1);
            int q = n_ent;
            if (tail_ref) { put(q, K_REF, t_start, t_src - t_start, -1, -1); ++q; }
            if (tail_pad) put(q, K_PAD_TRAIL, t_end, 0, -1, -1);
            meta[r].nseg = nseg; meta[r].npatch = npatch;
        }
        if (j >= nseg) pl.s_out[j] = 0x7FFFFFFF;       // sentinels for the 8-wide reads of P3b
        if (j >= npatch) pl.p_out[j] = 0x7FFFFFFF;
    }
    if (j == 0 && elig) meta[r].bad = ok ? 0 : 1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- P3b: lane = (row r, trip u = j) -------------------------------------------------
    if (ok && elig) {
        const int u = j;
        const int limit = hi_clip;
        const int p0 = lo_clip + u * TRIP;
        TripDesc &D = desc[r];
        int cls = 3, b1 = limit, b2 = limit, b3 = limit, idx = 0, pc0 = 0, pcn = 0;
        u32 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0, lo2 = 0, hi2 = 0, ldlo = 0, ldhi = 0;
        if (p0 < limit) {
            const int t_end2 = (limit - p0 > TRIP) ? p0 + TRIP : limit;
            {
                int so[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) so[t] = pl.s_out[t];
#pragma unroll
                for (int t = 1; t < 8; ++t) idx += (so[t] <= p0) ? 1 : 0;
                for (int s2 = 8; s2 < nseg; ++s2) idx += (pl.s_out[s2] <= p0) ? 1 : 0;
            }
            auto at = [&](int i) { return i < SEG_CAP ? i : SEG_CAP - 1; };
            b1 = idx + 1 < nseg ? pl.s_out[at(idx + 1)] : limit;
            b2 = idx + 2 < nseg ? pl.s_out[at(idx + 2)] : limit;
            b3 = idx + 3 < nseg ? pl.s_out[at(idx + 3)] : limit;
            lo0 = pl.s_lo[at(idx)]; hi0 = pl.s_hi[at(idx)];
            lo1 = pl.s_lo[at(idx + 1)]; hi1 = pl.s_hi[at(idx + 1)];
            lo2 = pl.s_lo[at(idx + 2)]; hi2 = pl.s_hi[at(idx + 2)];
            cls = b1 >= t_end2 ? 0 : (b2 >= t_end2 ? 1 : (b3 >= t_end2 ? 2 : 3));
            auto in_bounds = [&](u32 lo, u32 hi, int s, int e) {
                const u32 kind = hi >> 30;
                if (kind != K_REF && kind != K_ALLELE) return true;
                const i64 dl = seg_delta(lo, hi);
                const i64 len = kind == K_REF ? A.ref_len : A.alt_len;
                const int s3 = (s - 3 > p0 ? s - 3 : p0), e3 = (e + 3 < t_end2 ? e + 3 : t_end2);
                return dl + s3 >= 0 && dl + e3 <= len;
            };
            bool okb = in_bounds(lo0, hi0, p0, b1 < t_end2 ? b1 : t_end2);
            if (cls >= 1 && cls < 3) okb = okb && in_bounds(lo1, hi1, b1, b2 < t_end2 ? b2 : t_end2);
            if (cls == 2) okb = okb && in_bounds(lo2, hi2, b2, t_end2);
            if (!okb || ((t_end2 - p0) & 3) != 0 || (rflags & 4)) cls = 3;
            if (cls == 0) {
                const u32 kind = hi0 >> 30;
                if (kind == K_REF || kind == K_ALLELE) {
                    const u64 ad = (u64)(kind == K_REF ? A.ref : A.alt_alleles) + (u64)(seg_delta(lo0, hi0) + p0);
                    ldlo = (u32)ad; ldhi = (u32)(ad >> 32);
                } else {
                    cls = 3;
                }
            }
            {
                int po[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) po[t] = pl.p_out[t];
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    pc0 += (po[t] < p0) ? 1 : 0;
                    pcn += (po[t] < t_end2) ? 1 : 0;
                }
            }
        }
        D.cls[u] = cls; D.b1[u] = b1; D.b2[u] = b2; D.pc0[u] = pc0; D.pcn[u] = pcn; D.idx[u] = idx;
        D.ldlo[u] = ldlo; D.ldhi[u] = ldhi;
        D.lo0[u] = lo0; D.hi0[u] = hi0; D.lo1[u] = lo1; D.hi1[u] = hi1; D.lo2[u] = lo2; D.hi2[u] = hi2;
    }
    // release the rows' own waves (they poll meta[r].ready)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (elig && j == 0) __hip_atomic_store(&meta[r].ready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

#ifdef GVL_DIAG
#define GVL_STAMP(i) do { if (A.stamps && tid == 0) A.stamps[((u64)blockIdx.x * gridDim.y + blockIdx.y) * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define GVL_STAMP(i) do { } while (0)
#endif

template <bool ANNOT>
struct ReconShared {
    Luts luts;
    SegMirror mirror[WG_WAVES];
    Stage<ANNOT> stage[WG_WAVES];
    RowIn rin[WG_WAVES];
    RowPlan<ANNOT> plan[WG_WAVES];
    TripDesc desc[WG_WAVES];
    RowMeta meta[WG_WAVES];
    i32x4 lrec[WG_WAVES * GVL_SLOT_RECS];   // slot-major records of the 8 rows (read once, by wave 0)
};

// What one wave needs in LDS when it runs a row on its own (SOLO): the scalar walk's mirror only ever
// replaces a plan that failed, so the two share their memory.
template <bool ANNOT>
struct SoloLds {
    union { RowPlan<ANNOT> pl; SegMirror M; } u;
    Stage<ANNOT> G;
    RowIn ri;
};

// One workgroup's 8 (row, chunk)s: rows 8 wg .. 8 wg + 7 of the batch (S = the workgroup's tables).
// SOLO: ONE wave runs ONE row on its own -- the caller (recon_lean_kernel, for a row it cannot express)
// has put the row's parameters into solo->ri; no P1, no barrier, no packed plan: the row takes the
// per-wave scans (or the scalar walk) and streams from the byte reference like any row here.
template <int OH, bool HAPS, bool ANNOT, bool SOLO>
__device__ __forceinline__ void recon_body(const ReconArgs &A, ReconShared<ANNOT> *Sp, SoloLds<ANNOT> *solo, Luts &luts, const i64 wg, const int chunk) {
    SegMirror *const mirror = SOLO ? nullptr : Sp->mirror;
    Stage<ANNOT> *const stage = SOLO ? nullptr : Sp->stage;
    RowIn *const rin = SOLO ? nullptr : Sp->rin;
    RowPlan<ANNOT> *const plan = SOLO ? nullptr : Sp->plan;
    TripDesc *const desc = SOLO ? nullptr : Sp->desc;
    RowMeta *const meta = SOLO ? nullptr : Sp->meta;
    i32x4 *const lrec = SOLO ? nullptr : Sp->lrec;

    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = rfl(tid >> 6);
    const int lo_clip = chunk * A.chunk_len;
    const bool has_keep = A.keep && A.keep_offsets;
    const bool planned_ok = A.chunk_len <= CHUNK_TRIPS * TRIP && !(A.dbg & DBG_SCALAR_WALK);

    GVL_STAMP(0);
    if (!SOLO && tid < 256) {  // LUTs
        const u32 d = onehot_dword((u32)tid);
        luts.oh[tid] = d;
        luts.oh_rc[tid] = __builtin_bswap32(d);
        luts.comp[tid] = (u8)comp_byte((u32)tid);
    }
    // ---- P1 (wave 0): row parameters, one lane per row; then -- second memory level, side by side --
    // the contig bounds and the rows' slot-major variant records (lane = row x 8 + entry: the eight
    // 128-byte lines of the workgroup in ONE wave-load), all parked in LDS.  After the barrier no wave
    // needs a global read before its plan, so the reference bytes it requests next (below) stay in
    // flight behind nothing.
    const bool use_srec = !SOLO && A.srec != nullptr && !A.ref_only && planned_ok && !(A.dbg & DBG_NO_PACKABLE) && !ANNOT;
    // wave 0's carry from P1a to P1b (the slot-line read stays in flight across the first barrier)
    i32x4 p1_rec = {0, 0, (int)GVL_SREC_EMPTY, 0};
    i64 p1_oidx = 0;
    int p1_fl = 1;
    bool p1_want = false;
    if (!SOLO && tid < WAVE) {
        // Every load of a level is issued before anything waits (no branch in between: an absent
        // array is replaced by a pointer that is always readable, and a lane without a row reads
        // row 0), so P1 costs two memory round trips, not one per array.
        const i64 k_raw = wg * WG_WAVES + tid;
        const bool row_lane = tid < WG_WAVES && k_raw < A.n_rows;
        const i64 k = row_lane ? k_raw : 0;
        const i64 query = A.ploidy_shift >= 0 ? (k >> A.ploidy_shift) : (i64)((u32)k / (u32)A.ploidy);
        const int *reg = A.regions + query * A.regions_stride;
        const int *const dmy4 = A.regions;                                       // >= 12 readable bytes
        const i64 *const dmy8 = reinterpret_cast<const i64 *>(A.ref_offsets);    // >= 8 readable bytes
        // ---- level 1
        const int l_c = reg[0], l_start = reg[1], l_end = reg[2];
        const int l_shift = *(A.ref_only ? dmy4 : A.shifts + k);
        const i64 l_oidx = *(A.ref_only ? dmy8 : A.geno_offset_idx + k);
        const u8 l_rc = *(A.to_rc ? A.to_rc + k : reinterpret_cast<const u8 *>(dmy4));
        const i64 l_oo0 = *(A.out_offsets ? A.out_offsets + (k << A.oo_shift) : dmy8);
        const i64 l_oo1 = *(A.out_offsets ? A.out_offsets + (k << A.oo_shift) + 1 : dmy8);
        const i64 l_ko = *(has_keep && !A.ref_only ? A.keep_offsets + k : dmy8);
        RowIn ri;
        ri.c_s = ri.R = ri.o_s = 0;
        ri.n_var = 0;
        ri.k = (int)k;
        ri.ref_start = l_start;
        ri.shift = A.ref_only ? 0 : (i64)l_shift;
        ri.keep_off = (has_keep && !A.ref_only) ? l_ko : 0;
        ri.rc = A.to_rc ? (int)l_rc : 0;
        ri.row_base = A.out_offsets ? l_oo0 : k * A.fixed_len;
        ri.L = A.out_offsets ? (int)(l_oo1 - l_oo0) : (int)A.fixed_len;
        const i64 o_idx = A.ref_only ? 0 : l_oidx;
        int fl = 0;
        if (A.ref_only && (i64)l_start >= (i64)l_end) fl |= 4;                   // reference/mod.rs:16-18
        const bool shift_ok = !(ri.shift < 0 || ri.shift >= (1 << 30));
        if (!shift_ok || !planned_ok) fl |= 2;
        if (use_srec && shift_ok && !(A.dbg & GVL_ABL(DBG_ABL_NO_VARIANTS))) fl |= 16;
        // a row longer than the caller's max_row_len hint would be left partly unwritten: report it
        if (row_lane && chunk == 0 && A.async_err && (i64)ri.L > (i64)gridDim.y * (i64)A.chunk_len) *A.async_err = 1;
        if (!row_lane || lo_clip >= ri.L) fl = 1;
        if (row_lane && A.out_offsets_w && chunk == 0) {
            A.out_offsets_w[k] = ri.row_base;
            if (k == A.n_rows - 1) A.out_offsets_w[k + 1] = ri.row_base + ri.L;
        }
        // ---- level 2: contig bounds (L2 resident), CSR bounds (rows that do not use the slot-major
        // records), and LAST the rows' slot-major records, lane (r, j) = entry j of row r's slot: the
        // first two are waited for here, the slot lines stay in flight across the first barrier (P1b)
        const i64 c_idx = (l_c >= 0 && l_c < A.n_contigs) ? (i64)l_c : 0;       // (out of contract otherwise: clamp)
        const bool csr = !A.ref_only && !(fl & 17);
        const i64 o_safe = (csr && o_idx >= 0 && o_idx < A.n_geno_offsets) ? o_idx : 0;
        const i64 l_cs = A.ref_offsets[c_idx], l_ce = A.ref_offsets[c_idx + 1];
        const i64 l_gs = *(csr ? A.go_starts + o_safe : dmy8);
        const i64 l_ge = *(csr ? A.go_stops + o_safe : dmy8);
        if (use_srec) {
            const int r = lane >> 3;
            const int fl_r = bperm(r, fl);
            const u32 o_lo = (u32)bperm(r, (int)(u32)(u64)o_idx), o_hi = (u32)bperm(r, (int)(u32)((u64)o_idx >> 32));
            const i64 o_r = (i64)(((u64)o_hi << 32) | o_lo);
            p1_want = (fl_r & 17) == 16 && o_r >= 0 && o_r < A.n_geno_offsets;
            p1_rec = *reinterpret_cast<const i32x4 *>(A.srec + ((p1_want ? o_r : 0) * GVL_SLOT_RECS + (lane & 7)));
        }
        if (fl != 1) {
            ri.c_s = l_cs;
            ri.R = l_ce - l_cs;
            if (fl & 16) {
                // the variant count is known once the line is read (a slot with more than 8 falls
                // back to the CSR: P1b)
                ri.o_s = o_idx;
                ri.n_var = GVL_SLOT_RECS;
            } else if (csr) {
                ri.o_s = l_gs;
                const i64 nv = l_ge - l_gs;
                ri.n_var = nv < 0 ? 0 : (nv > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)nv);
                if (A.dbg & GVL_ABL(DBG_ABL_NO_VARIANTS)) ri.n_var = 0;
            }
            if (!(fl & 2) && ri.n_var <= 8 && !(A.dbg & DBG_NO_PACKABLE)) fl |= 8;           // packable: planned with the other rows
        }
        ri.flags = fl;
        p1_fl = fl; p1_oidx = o_idx;
        if (tid < WG_WAVES) {
            rin[tid] = ri;
            RowMeta m0; m0.nseg = m0.npatch = m0.bad = m0.slow = m0.ready = m0.pad0_ = m0.pad1_ = m0.pad2_ = 0;
            meta[tid] = m0;
        }
    }
    GVL_STAMP(1);
    if (!SOLO) lds_barrier();      // (not __syncthreads: its fence would wait for wave 0's slot-line read)
    // Every wave "uses" the slot-line registers here: a no-op for waves 1..7 (they have nothing in flight),
    // wave 0 needs the line next anyway.  Without it the compiler's wait-count model carries "a load into
    // these registers may be pending" past the reference reads below and, as soon as a register is reused,
    // waits for ALL of them (vmcnt(0) right after the second barrier).
    asm volatile("" :: "v"(p1_rec.x), "v"(p1_rec.y), "v"(p1_rec.z), "v"(p1_rec.w));

    GVL_STAMP(2);
    const RowIn &ri = SOLO ? solo->ri : rin[wave];
    int flags = rfl(ri.flags);
    const i64 k = SOLO ? (i64)rfl(ri.k) : wg * WG_WAVES + wave;
    RowPlan<ANNOT> &pl = SOLO ? solo->u.pl : plan[wave];
    Stage<ANNOT> &G = SOLO ? solo->G : stage[wave];
    const int L = rfl(ri.L);
    const i64 c_s = rfl64(ri.c_s);
    const int hi_clip = (L - lo_clip > A.chunk_len) ? lo_clip + A.chunk_len : L;
    int nseg = 0, npatch = 0;

    // ---- who plans this row ---------------------------------------------------------------
    //  * rows with at most 8 variants ("packable", flags & 8) read their records here, lane j =
    //    variant j.  If every kept variant is a SNP inside the contig and no two share a position
    //    the row is FAST: no scan is needed, its own wave plans it below and starts streaming
    //    while the others are still planning.
    //  * the other packable rows are SLOW: the first slow wave plans all of them at once
    //    (packed_plan), the other slow waves wait for their flag.
    //  * rows with more than 8 variants run the per-wave scans (P2 + P3 further down).
    bool packable = !SOLO && (flags & 11) == 8;
    int row_n_var = rfl(ri.n_var);        // (a slot-major row that overflows its line re-reads these from the CSR)
    i64 row_o_s = rfl64(ri.o_s);

    // ---- the "one reference run" reading of the row: n_lead pad bytes, then the contig from the
    // shifted origin r0, then pad.  It depends on the row parameters only, it is exact for a row
    // without indels and for the part of any row in front of its first indel -- so its reference
    // bytes are requested NOW, next to the variant records, instead of after the plan: one dependent
    // memory level less for SNP-only rows, and a prefetch into L2 for the others.
    int g_n_lead = 0, g_t_end = 0, g_r0 = 0; i64 g_delta = 0; bool g_ok = false;
    {
        const i64 rs = rfl64(ri.ref_start);
        if (!(flags & 3) && rs > -(1 << 30) && rs < (1 << 30)) {
            const int ref_start = (int)rs;
            const i64 R = rfl64(ri.R);
            const int shift_i = (int)rfl64(ri.shift);
            const int raw = ref_start < 0 ? -ref_start : 0;
            const int shifted0 = shift_i < raw ? shift_i : raw;
            g_n_lead = (raw - shifted0 < L) ? raw - shifted0 : L;
            g_r0 = (int)imin((i64)(ref_start < 0 ? 0 : ref_start) + (shift_i - shifted0), R);
            g_t_end = g_n_lead;
            const int u = L - g_n_lead;
            if (u > 0) {
                const int w = (int)imin((i64)u, R - g_r0);
                if (w > 0) g_t_end = g_n_lead + w;
            }
            g_delta = c_s + g_r0 - g_n_lead;
            g_ok = true;
        }
    }
    const int lane4 = GROUP * lane;
    // slot-major records of this row: parked in LDS by wave 0 (no global read, no vmcnt wait).  Then the
    // speculative reference reads: on the slot-major path nothing between here and pass A waits for a
    // global load, so they stay in flight while the row is classified and planned.
    bool ell = (flags & 16) != 0 && packable;        // (tentative until P1b has seen the slot line)
    const bool sp_on = g_ok && !(flags & 4) && !(A.dbg & (GVL_ABL(DBG_ABL_NO_LOADS) | DBG_NO_SPEC_REF)) && (ell || row_n_var == 0);
    // lane u decides for trip u (full trips only), one ballot; the loads then differ by an immediate
    // offset only.  (The scalar unit is shared by the waves of a CU: per-trip scalar arithmetic in the
    // head of every wave is what this avoids.)
    const u8 *const sp_base = A.ref + (g_delta + lo_clip) + (u32)lane4;
    u32 spmask = 0;
    if (sp_on) {
        const int p0 = lo_clip + lane * TRIP;
        const bool inside = lane < CHUNK_TRIPS && p0 >= g_n_lead && p0 + TRIP <= g_t_end && p0 + TRIP <= hi_clip &&
                            g_delta + p0 >= 0 && g_delta + p0 + TRIP <= A.ref_len;
        spmask = (u32)__builtin_amdgcn_ballot_w64(inside);
    }
    u32 wq[CHUNK_TRIPS];
    auto issue_spec = [&]() {
#pragma unroll
        for (int u = 0; u < CHUNK_TRIPS; ++u) {
            wq[u] = 0;
            if ((spmask >> u) & 1u) wq[u] = load_u32_unaligned(sp_base + u * TRIP);
        }
    };
    // waves 1..7 request their reference bytes NOW, under wave 0's slot-line read; wave 0 first parks the
    // slot lines (its own reads would otherwise sit in front of them: loads return in order)
    const bool spec_late = use_srec && wave == 0;
    if (!spec_late) issue_spec();
#ifdef GVL_DIAG
    // diagnostic (DBG_NO_FRONT): when do wave 1's speculative reference bytes arrive?  (stamp 15)
    if (A.stamps && (A.dbg & DBG_NO_FRONT) && wave == 1) {
        __builtin_amdgcn_s_waitcnt(0);
        if (lane == 0) A.stamps[((u64)blockIdx.x * gridDim.y + blockIdx.y) * 16 + 15] = __builtin_amdgcn_s_memrealtime();
    }
#endif

    // Who plans a row: see below (SNP-only rows plan themselves, the first wave that holds a row with
    // an indel plans all such rows of the workgroup).  Measured and dropped in round 2: wave 0 planning
    // EVERY packable row lane-parallel right after P1 while the other waves only keep their reference
    // reads in flight -- a third of the issue slots, but the packed plan is a 3.6 us chain of dependent
    // instructions when one wave runs it alone, and every row then waits for it (cfg3 14.5 vs 12.8 us,
    // cfg2 14.0 vs 12.0 us per launch on the same box).
    // ---- P1b (wave 0): the slot lines have arrived by now (they were requested before the reference
    // reads above, and loads return in order): park them in LDS; a slot with more than 8 variants sends
    // its row through the CSR (third level; rare).  Second LDS-only barrier.
    if (use_srec && tid < WAVE) {
        i32x4 rec = p1_rec;
        if (!p1_want) { rec.x = 0; rec.y = 0; rec.z = (int)GVL_SREC_EMPTY; rec.w = 0; }
        lrec[lane] = rec;
        const u64 ovf = __builtin_amdgcn_ballot_w64(p1_want && (lane & 7) == 0 && (u32)rec.z == GVL_SREC_OVERFLOW);
        if (ovf && tid < WG_WAVES && ((ovf >> (8 * tid)) & 1ull)) {
            const i64 gs = A.go_starts[p1_oidx];
            const i64 nv = A.go_stops[p1_oidx] - gs;
            rin[tid].o_s = gs;
            rin[tid].n_var = nv < 0 ? 0 : (nv > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)nv);
            rin[tid].flags = p1_fl & ~(8 | 16);          // more than 8 variants: not packable, per-wave scans
        }
    }
    if (use_srec) {
        lds_barrier();
        flags = rfl(ri.flags);
        packable = !SOLO && (flags & 11) == 8;
        row_n_var = rfl(ri.n_var);
        row_o_s = rfl64(ri.o_s);
        ell = (flags & 16) != 0 && packable;
    }
    if (spec_late) issue_spec();
    i32x4 srec_v = {0, 0, 0, 0};
    if (ell) srec_v = lrec[wave * GVL_SLOT_RECS + (lane & (GVL_SLOT_RECS - 1))];
    int f_pos = 0, f_inl = 0, f_vi = 0;
    bool f_valid = false, is_fast = false;
    if (packable) {
        int d = 0, alen = 0;
        bool rec_valid;
        if (ell) {
            const u32 e = (u32)srec_v.z;
            rec_valid = lane < GVL_SLOT_RECS && e != GVL_SREC_EMPTY;
            f_pos = srec_v.x; d = srec_v.y; alen = (int)(e >> 8); f_inl = (int)(e & 0xFF); f_vi = 0;
        } else {
            rec_valid = lane < row_n_var;
            if (rec_valid) {
                if (A.grec) {
                    const i32x4 rec = *reinterpret_cast<const i32x4 *>(A.grec + (row_o_s + lane));
                    f_pos = rec.x; d = rec.y; alen = (int)((u32)rec.z >> 8); f_inl = rec.z & 0xFF; f_vi = rec.w;
                } else {
                    int v = A.geno_v_idxs[row_o_s + lane];
                    v = v < 0 ? 0 : ((i64)v >= A.n_variants ? (int)(A.n_variants - 1) : v);
                    const i32x4 rec = *reinterpret_cast<const i32x4 *>(A.vrec + v);
                    f_pos = rec.x; d = rec.y; alen = rec.z; f_inl = rec.w & 0xFF; f_vi = v;
                }
            }
        }
        f_valid = rec_valid;
        if (f_valid && has_keep) f_valid = A.keep[rfl64(ri.keep_off) + lane] != 0;
        const i64 rs = rfl64(ri.ref_start);
        const int pos_prev = dpp_mov<0x138, 0xf>(-1, f_pos);               // wave_shr:1
        const u64 m_slow = __builtin_amdgcn_ballot_w64(
            (f_valid && (d != 0 || alen != 1 || f_pos < 0 || (i64)f_pos + 1 > rfl64(ri.R))) ||
            (lane > 0 && rec_valid && f_pos == pos_prev));
        is_fast = packable && m_slow == 0 && rs > -(1 << 30) && rs < (1 << 30) && !(A.dbg & DBG_NO_SNP_PLAN);
        // tell the workgroup: the slow flag, then one tick of the "decided" counter (meta[0].pad0_)
        if (lane == 0) {
            if (packable && !is_fast) meta[wave].slow = 1;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __hip_atomic_fetch_add(&meta[0].pad0_, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    GVL_STAMP(3);
    // Fast rows go on at once.  A slow row waits until every packable row has decided (no
    // workgroup barrier: the fast waves must not wait for anybody), then the first slow wave
    // plans all slow rows and the others poll their flag.
    const bool slow_row = packable && !is_fast;
    if (slow_row) {
        const int n_packable = __builtin_popcountll(
            __builtin_amdgcn_ballot_w64(lane < WG_WAVES && (rin[lane < WG_WAVES ? lane : 0].flags & 11) == 8));
        while (__hip_atomic_load(&meta[0].pad0_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < n_packable)
            __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const u64 m_slow_rows = __builtin_amdgcn_ballot_w64(lane < WG_WAVES && meta[lane < WG_WAVES ? lane : 0].slow != 0);
        if (wave == __builtin_ctzll(m_slow_rows)) {
            __builtin_amdgcn_s_setprio(3);      // the other slow rows wait for this wave
            packed_plan<ANNOT>(A, rin, plan, desc, meta, lrec, lane, lo_clip, has_keep);
        } else {
            while (__hip_atomic_load(&meta[wave].ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0)
                __builtin_amdgcn_s_sleep(2);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    const bool packed = slow_row;
    const bool fast_row = packable && is_fast;
    int fp_n_lead = 0, fp_t_end = 0, fp_lead_kept = 0; bool fp_ref = false, fp_pad = false; i64 fp_delta = 0;

    if (fast_row) {
        // ---- fast plan: ONE reference run from the shifted origin r0 + SNP patches.  With SNPs only,
        // whichever way the shift completes (:115-146) or runs out (:200-205), ref_idx lands on
        // ref_idx0 + shift; SNP i sits at n_lead + (pos_i - r0) iff pos_i >= r0 and that is
        // inside the row (:154-158).
        const int n_lead = g_n_lead, r0 = g_r0, t_end = g_t_end;      // (is_fast implies g_ok)
        const int ao = n_lead + (f_pos - r0);
        const bool app = f_valid && f_pos >= r0 && (f_pos - r0) < (L - n_lead);
        const u64 m_p = __builtin_amdgcn_ballot_w64(app && ao >= lo_clip && ao < hi_clip);
        if ((m_p >> lane) & 1ull) {
            const int ps = __builtin_popcountll(m_p & ((1ull << lane) - 1ull));
            pl.p_out[ps] = ao; pl.p_val[ps] = f_inl;
            if (ANNOT) pl.p_id[ps] = f_vi;
        }
        npatch = __builtin_popcountll(m_p);
        const int lead_kept = (n_lead > 0 && n_lead > lo_clip && 0 < hi_clip) ? 1 : 0;
        const bool tail_pad = t_end < L && L > lo_clip && t_end < hi_clip;
        const bool tail_ref = t_end > n_lead && t_end > lo_clip && n_lead < hi_clip;
        nseg = lead_kept + (tail_ref ? 1 : 0) + (tail_pad ? 1 : 0);
        fp_n_lead = n_lead; fp_t_end = t_end; fp_lead_kept = lead_kept; fp_ref = tail_ref; fp_pad = tail_pad;
        fp_delta = c_s + r0 - n_lead;
        if (lane == 0) {
            auto put1 = [&](int q, u32 kind, int o_start, i64 delta) {
                const u64 e = (u64)(delta + DELTA_BIAS) | ((u64)kind << 62);
                pl.s_out[q] = o_start; pl.s_lo[q] = (u32)e; pl.s_hi[q] = (u32)(e >> 32);
                if (ANNOT) { pl.s_a[q] = -1; pl.s_b[q] = -1; }
            };
            int q = 0;
            if (lead_kept) { put1(q, K_PAD_LEAD, 0, 0); ++q; }
            if (tail_ref) { put1(q, K_REF, n_lead, c_s + r0 - n_lead); ++q; }
            if (tail_pad) put1(q, K_PAD_TRAIL, t_end, 0);
        }
        if (lane < 8) {
            if (lane >= nseg) pl.s_out[lane] = 0x7FFFFFFF;
            if (lane >= npatch) pl.p_out[lane] = 0x7FFFFFFF;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    if (!(flags & 3) && !packable) {
        // ---- P2 + P3, 64 variants per trip with carries between trips ------------------------
        const int n_var = row_n_var;
        const i64 o_s = row_o_s;
        const int ref_start = (int)rfl64(ri.ref_start);
        const i64 R = rfl64(ri.R);
        const i64 keep_off = has_keep ? rfl64(ri.keep_off) : 0;
        bool ok = ref_start > -(1 << 30) && ref_start < (1 << 30);
        // leading pad absorbs the shift first (:68-83)
        const int shift_i = (int)rfl64(ri.shift);
        const int raw = ref_start < 0 ? -ref_start : 0;
        const int shifted0 = shift_i < raw ? shift_i : raw;
        const int n_lead = (raw - shifted0 < L) ? raw - shifted0 : L;
        int rem = shift_i - shifted0;                  // shift still open
        int ref_idx0 = ref_start < 0 ? 0 : ref_start;  // ref_idx before the first applied variant
        int pm_carry = ref_idx0;                       // max(ref_idx0, v_end of every applied variant so far)
        int x_carry = 0;                               // output bases produced by the applied variants so far
        bool ended = false;                            // the ">= L" break has happened
        bool have_ns = false; int ns_end = 0, ns_E = 0;   // last applied indel: allele end (out), v_end (ref)
        int ref_idx_end = ref_idx0, out_idx_end = n_lead; // walk state after the last applied variant
        bool any_applied = false;
        const int lead_kept = (n_lead > 0 && n_lead > lo_clip && 0 < hi_clip) ? 1 : 0;
        int n_ent = lead_kept;
        bool past_chunk = false;                       // every later variant lands at or after hi_clip
        auto enc = [](u32 kind, i64 delta, u32 &lo, u32 &hi) {
            const u64 e = (u64)(delta + DELTA_BIAS) | ((u64)kind << 62);
            lo = (u32)e; hi = (u32)(e >> 32);
        };
        auto put = [&](int q, u32 kind, int o_start, i64 delta, int id, int vpos) {
            if (q < SEG_CAP) {
                u32 lo, hi; enc(kind, delta, lo, hi);
                pl.s_out[q] = o_start; pl.s_lo[q] = lo; pl.s_hi[q] = hi;
                if (ANNOT) { pl.s_a[q] = id; pl.s_b[q] = vpos; }
            }
        };

        for (int tb = 0; tb < n_var && ok && !ended && !past_chunk; tb += WAVE) {
            int pos = 0, d = 0, alen = 0, inl = 0, vi = 0; i64 a0 = 0;
            bool valid = tb + lane < n_var;
            if (valid) {
                if (A.grec) {
                    // the variant's fields sit next to the CSR entry: one contiguous read, and
                    // only lanes that will need allele bytes from memory go on to alt_offsets
                    const i32x4 rec = *reinterpret_cast<const i32x4 *>(A.grec + (o_s + tb + lane));
                    pos = rec.x; d = rec.y; alen = (int)((u32)rec.z >> 8); inl = rec.z & 0xFF; vi = rec.w;
                    if (!(d == 0 && alen == 1)) a0 = A.alt_offsets[vi];
                } else {
                    int v = A.geno_v_idxs[o_s + tb + lane];
                    v = v < 0 ? 0 : ((i64)v >= A.n_variants ? (int)(A.n_variants - 1) : v);
                    const i32x4 rec = *reinterpret_cast<const i32x4 *>(A.vrec + v);
                    a0 = A.alt_offsets[v];
                    pos = rec.x; d = rec.y; alen = rec.z; inl = rec.w; vi = v;
                }
                if (has_keep) valid = A.keep[keep_off + tb + lane] != 0;
            }
            // coordinates beyond 2^30 (or nonsense) go to the scalar path: everything below is i32
            // (grec clips alen to 2^24 - 1: such an allele is "weird" here and exact there)
            const bool weird = valid && (pos < 0 || pos >= (1 << 30) || d <= -(1 << 30) || d >= (1 << 30) ||
                                         alen < 0 || alen >= (A.grec ? 0xFFFFFF : (1 << 30)));
            ok = ok && __builtin_amdgcn_ballot_w64(weird) == 0;
            const int E = pos - (d < 0 ? d : 0) + 1;                        // v_ref_end, :96
            const bool is_snp = d == 0 && alen == 1;
            // DEL spanning the window start (:99-102): the last one in order sets ref_idx.  Such
            // variants precede every candidate (sorted by position), so nothing is applied yet.
            // a row with an indel has the longest plan and the slowest trips; it decides when the
            // launch ends, so its wave wins the issue arbitration against waves already streaming
            // (cfg3: -0.4..-0.7 us per launch, nothing lost with several batches in flight)
            if (__builtin_amdgcn_ballot_w64(valid && !is_snp)) __builtin_amdgcn_s_setprio(3);
            const u64 m_span = __builtin_amdgcn_ballot_w64(valid && pos < ref_start && d < 0 && E >= ref_start);
            if (m_span) { ref_idx0 = rdl(E, 63 - __builtin_clzll(m_span)); pm_carry = ref_idx0; ref_idx_end = ref_idx0; }
            bool cand = valid && pos >= ref_start;
            // shift consumption (:115-146).  While the shift is open ref_idx stays put, so the
            // variants in front of the one that completes it are simply dropped; that one (lane f)
            // either starts after the shifted origin, or loses the first `skip` bytes of its
            // allele, or is consumed entirely.
            if (rem > 0) {
                const int base = ref_idx0;
                const u64 m_t = __builtin_amdgcn_ballot_w64(cand && pos >= base && (pos - base) + alen >= rem);
                if (m_t == 0) {
                    cand = false;                      // still open after this trip
                } else {
                    const int f = __builtin_ctzll(m_t);
                    const int dist = rdl(pos, f) - base;
                    if (dist >= rem) {
                        ref_idx0 = base + rem;
                        cand = cand && lane >= f;
                    } else {
                        const int skip = rem - dist;
                        if (skip == rdl(alen, f)) {
                            ref_idx0 = rdl(E, f);
                            cand = cand && lane > f;
                        } else {
                            ref_idx0 = rdl(pos, f);
                            cand = cand && lane >= f;
                            if (lane == f) { alen -= skip; a0 += skip; }
                        }
                    }
                    rem = 0;
                    pm_carry = ref_idx0; ref_idx_end = ref_idx0;
                }
            }
            // first ALT wins (:108-110): fixed point of B = {i : pos_i >= max(carry, max E over B before i)}
            bool inB = cand;
            int PM = 0, pm_incl = 0;
            {
                u64 mB = __builtin_amdgcn_ballot_w64(inB);
                bool stable = false;
#pragma unroll 1
                for (int it = 0; it < 4 && !stable; ++it) {
                    PM = wave_scan_exclusive<OpMaxU>(inB ? E : 0, pm_incl);
                    PM = PM > pm_carry ? PM : pm_carry;
                    inB = cand && pos >= PM;
                    const u64 m2 = __builtin_amdgcn_ballot_w64(inB);
                    stable = m2 == mB;
                    mB = m2;
                }
                ok = ok && stable;
            }
            // output offsets: exclusive prefix sum of (reference run + allele)      (the indel shift)
            const int n_i = inB ? pos - PM : 0;
            const int S_i = inB ? OpSat::f(n_i, alen) : 0;
            int x_incl;
            const int X = OpSat::f(x_carry, wave_scan_exclusive<OpSat>(S_i, x_incl));
            const int allele_out = OpSat::f(OpSat::f(n_lead, X), n_i);
            const bool applied = inB && allele_out < L;                       // :154-158 break
            const int w_i = applied ? ((alen < L - allele_out) ? alen : L - allele_out) : 0;   // :178
            const bool nonsnp = applied && !is_snp;
            const bool snp = applied && is_snp;
            const u64 m_inB = __builtin_amdgcn_ballot_w64(inB);
            const u64 m_app = __builtin_amdgcn_ballot_w64(applied);
            if (m_inB != m_app) ended = true;
            if (m_app) {
                const int last = 63 - __builtin_clzll(m_app);
                ref_idx_end = rdl(E, last);
                out_idx_end = rdl(allele_out, last) + rdl(w_i, last);
                any_applied = true;
                if (rdl(allele_out, last) >= hi_clip) past_chunk = true;
            }
            // the reference run in front of each applied indel starts after the previous applied indel
            const int prevNS = wave_scan_exclusive<OpMaxI>(nonsnp ? lane : -1);
            const int pidx = prevNS < 0 ? 0 : prevNS;
            const int p_end = bperm(pidx, allele_out + alen);                 // not truncated: it has a successor
            const int p_E = bperm(pidx, E);
            const int run_start = prevNS < 0 ? (have_ns ? ns_end : n_lead) : p_end;
            const i64 run_src = c_s + (prevNS < 0 ? (have_ns ? ns_E : ref_idx0) : p_E);
            const bool e_ref = nonsnp && allele_out > run_start && allele_out > lo_clip && run_start < hi_clip;
            const bool e_all = nonsnp && w_i > 0 && allele_out + w_i > lo_clip && allele_out < hi_clip;
            const int slot0 = n_ent + wave_scan_exclusive<OpAdd>((e_ref ? 1 : 0) + (e_all ? 1 : 0));
            const u64 m_ns = __builtin_amdgcn_ballot_w64(nonsnp);
            const u64 m_snp = __builtin_amdgcn_ballot_w64(snp && allele_out >= lo_clip && allele_out < hi_clip);
            const int add_ent = __builtin_popcountll(__builtin_amdgcn_ballot_w64(e_ref)) +
                                __builtin_popcountll(__builtin_amdgcn_ballot_w64(e_all));
            const int add_pat = __builtin_popcountll(m_snp);
            if (n_ent + add_ent + 2 > SEG_CAP || npatch + add_pat > WAVE) ok = false;
            if (ok) {
                int q = slot0;
                if (e_ref) { put(q, K_REF, run_start, run_src - run_start, -1, -1); ++q; }
                if (e_all) put(q, K_ALLELE, allele_out, a0 - allele_out, vi, pos);
                if ((m_snp >> lane) & 1ull) {
                    const int ps = npatch + __builtin_popcountll(m_snp & ((1ull << lane) - 1ull));
                    pl.p_out[ps] = allele_out; pl.p_val[ps] = inl & 0xFF;
                    if (ANNOT) pl.p_id[ps] = vi;
                }
            }
            // carries
            if (tb + WAVE < n_var) {
                // pm_incl is the scan of the last fixed-point round, whose input mask equals
                // the final one (that is what "stable" means)
                const int mx = rdl(pm_incl, 63);
                pm_carry = mx > pm_carry ? mx : pm_carry;
                x_carry = OpSat::f(x_carry, rdl(x_incl, 63));
            }
            if (m_ns) {
                const int last = 63 - __builtin_clzll(m_ns);
                ns_end = rdl(allele_out, last) + rdl(alen, last);
                ns_E = rdl(E, last);
                have_ns = true;
            }
            n_ent += add_ent;
            npatch += add_pat;
        }
        if (ok) {
            // the run after the last applied indel (through any SNPs), then -- if the walk ran to
            // its end -- the rest of the contig and the right pad (:200-255)
            if (rem > 0) ref_idx_end = (int)imin((i64)ref_idx0 + rem, R);     // shift never completed
            const int t_start = have_ns ? ns_end : n_lead;
            const i64 t_src = c_s + (have_ns ? ns_E : ((rem > 0 && !any_applied) ? ref_idx_end : ref_idx0));
            int t_end = out_idx_end;
            bool tail_pad = false;
            if (past_chunk && !ended) {
                t_end = hi_clip;                        // open run: covers the rest of this chunk
            } else {
                const int u = L - out_idx_end;
                if (u > 0) {
                    const i64 avail = R - ref_idx_end;
                    const int w = (int)imin((i64)u, avail);
                    if (w > 0) t_end = out_idx_end + w;
                }
                tail_pad = t_end < L && L > lo_clip && t_end < hi_clip;
            }
            const bool tail_ref = t_end > t_start && t_end > lo_clip && t_start < hi_clip;
            if (lane == 0) {
                if (lead_kept) put(0, K_PAD_LEAD, 0, 0, -1, -1);
                int q = n_ent;
                if (tail_ref) { put(q, K_REF, t_start, t_src - t_start, -1, -1); ++q; }
                if (tail_pad) put(q, K_PAD_TRAIL, t_end, 0, -1, -1);
            }
            nseg = n_ent + (tail_ref ? 1 : 0) + (tail_pad ? 1 : 0);
            // sentinels: P3b counts starts <= p0 over the first 8 slots without bounds checks
            if (lane < 8) {
                if (lane >= nseg) pl.s_out[lane] = 0x7FFFFFFF;
                if (lane >= npatch) pl.p_out[lane] = 0x7FFFFFFF;
            }
        } else {
            flags |= 2;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (flags & 1) return;
    if (!SOLO && packed) {
        if (rfl(meta[wave].bad)) flags |= 2;
        nseg = rfl(meta[wave].nseg); npatch = rfl(meta[wave].npatch);
    }
    GVL_STAMP(4);
#ifdef GVL_DIAG
    if (A.stamps && lane == 0 && (flags & 2)) atomicAdd((unsigned long long *)&A.stamps[((u64)blockIdx.x * gridDim.y + blockIdx.y) * 16 + 9], 1ull);
#endif
    if (flags & 2) {
        recon_wave_scalar<OH, HAPS, ANNOT>(A, luts, SOLO ? solo->u.M : mirror[wave], G, k, chunk, lane);
        return;
    }

    // ---- P3b: trip descriptors, lane u = trip u of this row -------------------------------
    // A trip (256 bases) is described by the <= 3 table entries that cover it (class 0..2 =
    // 1..3 entries; the typical indel trip is REF | ALLELE | REF); anything else (4+ entries,
    // a source that would be read past an array end, the partial last group, zero fill) is
    // class 3 = general.  Entry j spans [b_j, b_{j+1}) with b_0 <= p0.
    const bool ref_zero_fill = (flags & 4) != 0;
    const int limit = hi_clip;
    int d_cls = 3, d_b1 = 0, d_b2 = 0, d_pc0 = 0, d_pcn = 0, d_idx = 0;
    u32 d_ldlo = 0, d_ldhi = 0;     // class 0: address of the trip's first source byte
    u32 d_lo0 = 0, d_hi0 = 0, d_lo1 = 0, d_hi1 = 0, d_lo2 = 0, d_hi2 = 0;
    if (!SOLO && packed) {
        if (lane < CHUNK_TRIPS) {
            const TripDesc &D = desc[wave];
            d_cls = D.cls[lane]; d_b1 = D.b1[lane]; d_b2 = D.b2[lane]; d_pc0 = D.pc0[lane]; d_pcn = D.pcn[lane];
            d_idx = D.idx[lane]; d_ldlo = D.ldlo[lane]; d_ldhi = D.ldhi[lane];
            d_lo0 = D.lo0[lane]; d_hi0 = D.hi0[lane]; d_lo1 = D.lo1[lane]; d_hi1 = D.hi1[lane];
            d_lo2 = D.lo2[lane]; d_hi2 = D.hi2[lane];
        }
    } else if (fast_row) {
        // one reference run (+ pads at a contig edge): a trip inside the run is class 0 with a known
        // address, any other trip is general
        if (lane < CHUNK_TRIPS) {
            const int p0 = lo_clip + lane * TRIP;
            if (p0 < limit) {
                const int t_end = (limit - p0 > TRIP) ? p0 + TRIP : limit;
                d_idx = fp_lead_kept + ((fp_ref && fp_n_lead <= p0) ? 1 : 0) + ((fp_pad && fp_t_end <= p0) ? 1 : 0) - 1;
                if (d_idx < 0) d_idx = 0;
                d_b1 = limit; d_b2 = limit;
                const bool inside = fp_ref && p0 >= fp_n_lead && t_end <= fp_t_end && fp_delta + p0 >= 0 &&
                                    fp_delta + t_end <= A.ref_len && ((t_end - p0) & 3) == 0 && !ref_zero_fill;
                if (inside) {
                    d_cls = 0;
                    const u64 ad = (u64)A.ref + (u64)(fp_delta + p0);
                    d_ldlo = (u32)ad; d_ldhi = (u32)(ad >> 32);
                    if (ANNOT) {
                        const u64 e = (u64)(fp_delta + DELTA_BIAS) | ((u64)K_REF << 62);
                        d_lo0 = (u32)e; d_hi0 = (u32)(e >> 32);
                    }
                }
                if (npatch > 0) {
                    int po[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) po[j] = pl.p_out[j];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        d_pc0 += (po[j] < p0) ? 1 : 0;
                        d_pcn += (po[j] < t_end) ? 1 : 0;
                    }
                }
            }
        }
    } else if (lane < CHUNK_TRIPS) {
        const int p0 = lo_clip + lane * TRIP;
        if (p0 < limit) {
            const int t_end = (limit - p0 > TRIP) ? p0 + TRIP : limit;
            // entry holding p0 = (#entries starting at or before p0) - 1.  The first 8 starts are
            // read in one go (independent LDS reads); longer tables continue with a loop.
            int idx = 0;
            {
                int so[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) so[j] = pl.s_out[j];
#pragma unroll
                for (int j = 1; j < 8; ++j) idx += (so[j] <= p0) ? 1 : 0;
                for (int s2 = 8; s2 < nseg; ++s2) idx += (pl.s_out[s2] <= p0) ? 1 : 0;
            }
            auto at = [&](int i) { return i < SEG_CAP ? i : SEG_CAP - 1; };
            const int b1 = idx + 1 < nseg ? pl.s_out[at(idx + 1)] : limit;
            const int b2 = idx + 2 < nseg ? pl.s_out[at(idx + 2)] : limit;
            const int b3 = idx + 3 < nseg ? pl.s_out[at(idx + 3)] : limit;
            d_lo0 = pl.s_lo[at(idx)]; d_hi0 = pl.s_hi[at(idx)];
            d_lo1 = pl.s_lo[at(idx + 1)]; d_hi1 = pl.s_hi[at(idx + 1)];
            d_lo2 = pl.s_lo[at(idx + 2)]; d_hi2 = pl.s_hi[at(idx + 2)];
            int cls = b1 >= t_end ? 0 : (b2 >= t_end ? 1 : (b3 >= t_end ? 2 : 3));
            // every group that overlaps entry j loads the dword at delta_j + p, i.e. up to 3
            // bytes before/after the entry's own span: those must stay inside the array
            auto in_bounds = [&](u32 lo, u32 hi, int s, int e) {
                const u32 kind = hi >> 30;
                if (kind != K_REF && kind != K_ALLELE) return true;
                const i64 dl = seg_delta(lo, hi);
                const i64 len = kind == K_REF ? A.ref_len : A.alt_len;
                const int s3 = (s - 3 > p0 ? s - 3 : p0), e3 = (e + 3 < t_end ? e + 3 : t_end);
                return dl + s3 >= 0 && dl + e3 <= len;
            };
            bool okb = in_bounds(d_lo0, d_hi0, p0, b1 < t_end ? b1 : t_end);
            if (cls >= 1 && cls < 3) okb = okb && in_bounds(d_lo1, d_hi1, b1, b2 < t_end ? b2 : t_end);
            if (cls == 2) okb = okb && in_bounds(d_lo2, d_hi2, b2, t_end);
            if (!okb || ((t_end - p0) & 3) != 0 || ref_zero_fill) cls = 3;
            if (cls == 0) {
                const u32 kind = d_hi0 >> 30;
                if (kind == K_REF || kind == K_ALLELE) {
                    const u64 ad = (u64)(kind == K_REF ? A.ref : A.alt_alleles) + (u64)(seg_delta(d_lo0, d_hi0) + p0);
                    d_ldlo = (u32)ad; d_ldhi = (u32)(ad >> 32);
                } else {
                    cls = 3;    // a trip of pure padding: rare, the general path writes it
                }
            }
            {
                int po[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) po[j] = pl.p_out[j];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    d_pc0 += (po[j] < p0) ? 1 : 0;
                    d_pcn += (po[j] < t_end) ? 1 : 0;
                }
                for (int q = 8; q < npatch; ++q) {
                    const int pp = pl.p_out[q];
                    d_pc0 += pp < p0 ? 1 : 0;
                    d_pcn += pp < t_end ? 1 : 0;
                }
            }
            d_cls = cls; d_b1 = b1; d_b2 = b2; d_idx = idx;
        }
    }
    GVL_STAMP(5);
#ifdef GVL_DIAG
    if (A.stamps && lane == 0) {   // every wave: latest / earliest "plan ready"
        unsigned long long *b = (unsigned long long *)&A.stamps[((u64)blockIdx.x * gridDim.y + blockIdx.y) * 16];
        const unsigned long long t = __builtin_amdgcn_s_memrealtime();
        atomicMax(b + 13, t);
        atomicMin(b + 14, t);
    }
#endif

    // ---- P4: stream ----------------------------------------------------------------------
    const bool rc = rfl(ri.rc) != 0;
    const i64 row_base = rfl64(ri.row_base);
    const u32 padb = A.pad & 0xFFu;
    const u32 rc_sel = rc ? 0x00010203u : 0x03020100u;
    const u32 *oh_t = rc ? luts.oh_rc : luts.oh;
    const int lane_pos = rc ? -GROUP * lane : GROUP * lane;
    u8 *hap_row = HAPS ? A.haps + row_base : nullptr;
    u8 *oh_row = OH != OH_NONE ? A.onehot + 4 * row_base : nullptr;
    int *av_row = (ANNOT && A.av) ? A.av + row_base : nullptr;
    int *ap_row = (ANNOT && A.ap) ? A.ap + row_base : nullptr;

    // finish one trip: SNP patches, reverse-complement, one-hot LUT, stores
    auto finish = [&](const int p0, const int pc0, const int pcn, u32 wv, int (&av4)[GROUP], int (&ap4)[GROUP]) -> u32 {
        const int p = p0 + GROUP * lane;
        const bool full = p + GROUP <= limit;
        for (int q = pc0; q < pcn; ++q) {
            const u32 dd = (u32)(pl.p_out[q] - p);
            if (dd < (u32)GROUP) {
                const u32 sh = dd * 8;
                wv = (wv & ~(0xFFu << sh)) | ((u32)pl.p_val[q] << sh);
            }
            if (ANNOT) {
                const int pid = pl.p_id[q];
#pragma unroll
                for (int i = 0; i < GROUP; ++i) if (dd == (u32)i) av4[i] = pid;
            }
        }
        if (full && !(A.dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
            const int jo = (rc ? L - GROUP - p0 : p0) + lane_pos;
            const u32 ww = __builtin_amdgcn_perm(0u, wv, rc_sel);
            const u32 b0_ = ww & 0xFF, b1_ = (ww >> 8) & 0xFF, b2_ = (ww >> 16) & 0xFF, b3_ = ww >> 24;
            if (OH == OH_LC) {
                u32x4_a4 o = {oh_t[b0_], oh_t[b1_], oh_t[b2_], oh_t[b3_]};
                store_oh16(oh_row + 4 * (i64)jo, o);
            } else if (OH == OH_CL) {
                const u32 d0 = oh_t[b0_], d1 = oh_t[b1_], d2 = oh_t[b2_], d3 = oh_t[b3_];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const u32 sh = 8 * a;
                    const u32 v = ((d0 >> sh) & 0xFF) | (((d1 >> sh) & 0xFF) << 8) |
                                  (((d2 >> sh) & 0xFF) << 16) | (((d3 >> sh) & 0xFF) << 24);
                    store_u32_unaligned(oh_row + (i64)a * L + jo, v);
                }
            }
            if (HAPS) {
                u32 hv = ww;
                if (rc) hv = (u32)luts.comp[b0_] | ((u32)luts.comp[b1_] << 8) | ((u32)luts.comp[b2_] << 16) | ((u32)luts.comp[b3_] << 24);
                store_u32_unaligned(hap_row + jo, hv);
            }
            if (ANNOT) {
                if (av_row) {
                    i32x4_a4 o = rc ? i32x4_a4{av4[3], av4[2], av4[1], av4[0]} : i32x4_a4{av4[0], av4[1], av4[2], av4[3]};
                    store_i32x4(av_row + jo, o.x, o.y, o.z, o.w);
                }
                if (ap_row) {
                    i32x4_a4 o = rc ? i32x4_a4{ap4[3], ap4[2], ap4[1], ap4[0]} : i32x4_a4{ap4[0], ap4[1], ap4[2], ap4[3]};
                    store_i32x4(ap_row + jo, o.x, o.y, o.z, o.w);
                }
            }
        }
        return wv;
    };

    // the partial group at the row end (L % 4 != 0) -- only class-3 trips can hold it
    auto finish_partial = [&](const int p0, const u32 wv, int (&av4)[GROUP], int (&ap4)[GROUP]) {
        const int p = p0 + GROUP * lane;
        const bool act = p < limit;
        const bool full = p + GROUP <= limit;
        if (limit & 3) {
            // partial group at the row end (L % 4 != 0): per-base stores by lanes 0..(L&3)-1
            const int p_last = limit & ~3;
            if (p_last >= p0 && p_last < p0 + TRIP) {
                if (act && !full) {
                    G.w[0] = wv;
                    if (ANNOT) {
#pragma unroll
                        for (int i = 0; i < GROUP; ++i) { G.av[i][0] = av4[i]; G.ap[i][0] = ap4[i]; }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (lane < (limit & 3)) {
                    const int pp = p_last + lane;
                    const u32 b = (G.w[0] >> (8 * lane)) & 0xFF;
                    const i64 jo = rc ? (i64)(L - 1 - pp) : (i64)pp;
                    if (OH != OH_NONE) {
                        const u32 dd = oh_t[b];
                        if (OH == OH_LC) {
                            __builtin_memcpy(oh_row + 4 * jo, &dd, 4);
                        } else {
#pragma unroll
                            for (int a = 0; a < 4; ++a) oh_row[(i64)a * L + jo] = (u8)((dd >> (8 * a)) & 0xFF);
                        }
                    }
                    if (HAPS) hap_row[jo] = (u8)(rc ? luts.comp[b] : b);
                    if (ANNOT) {
                        if (av_row) av_row[jo] = G.av[lane][0];
                        if (ap_row) ap_row[jo] = G.ap[lane][0];
                    }
                }
            }
        }
    };

    // Trip classes: 0 = one entry (uniform), 1/2 = two/three entries ("multi": the typical
    // indel trip), 3 = general.  Loads are issued in the order multi (up to 2 trips), then
    // all class-0 trips, so that everything is in flight before the first wait.
    auto entry_load = [&](const u32 lo, const u32 hi, const int p, const bool pred) -> u32 {
        const u32 kind = hi >> 30;                       // uniform
        if (kind == K_REF || kind == K_ALLELE) {
            const u8 *arr = (kind == K_REF ? A.ref : A.alt_alleles) + seg_delta(lo, hi);
            u32 v = 0;
            if (pred && !(A.dbg & GVL_ABL(DBG_ABL_NO_LOADS))) v = load_u32_unaligned(arr + p);
            return v;
        }
        return padb * 0x01010101u;
    };
    auto bytes_below = [](int k) -> u32 { return k <= 0 ? 0u : (k >= 4 ? 0xFFFFFFFFu : ((1u << (8 * k)) - 1u)); };
    auto multi_issue = [&](const int u, u32 (&w3)[3]) {
        const int p = lo_clip + u * TRIP + GROUP * lane;
        const int cls = rdl(d_cls, u);
        const int b1 = rdl(d_b1, u), b2 = rdl(d_b2, u);
        w3[0] = entry_load((u32)rdl((int)d_lo0, u), (u32)rdl((int)d_hi0, u), p, p < limit && p < b1);
        w3[1] = entry_load((u32)rdl((int)d_lo1, u), (u32)rdl((int)d_hi1, u), p, p < limit && p + GROUP > b1 && p < b2);
        w3[2] = 0;
        if (cls >= 2) w3[2] = entry_load((u32)rdl((int)d_lo2, u), (u32)rdl((int)d_hi2, u), p, p < limit && p + GROUP > b2);
    };
    auto multi_finish = [&](const int u, const u32 (&w3)[3]) {
        const int p0 = lo_clip + u * TRIP;
        const int p = p0 + GROUP * lane;
        const int cls = rdl(d_cls, u);
        const int b1 = rdl(d_b1, u), b2 = rdl(d_b2, u);
        const u32 m1 = bytes_below(b1 - p);           // bytes of entry 0
        const u32 m2 = bytes_below(b2 - p);           // bytes of entries 0 and 1
        const u32 wv = (w3[0] & m1) | (w3[1] & m2 & ~m1) | (w3[2] & ~m2);
        int av4[GROUP], ap4[GROUP];
        if (ANNOT) {
            const u32 lo_[3] = {(u32)rdl((int)d_lo0, u), (u32)rdl((int)d_lo1, u), (u32)rdl((int)d_lo2, u)};
            const u32 hi_[3] = {(u32)rdl((int)d_hi0, u), (u32)rdl((int)d_hi1, u), (u32)rdl((int)d_hi2, u)};
            const int i0 = rdl(d_idx, u);
#pragma unroll
            for (int i = 0; i < GROUP; ++i) {
                const int pp = p + i;
                const int j = pp >= b1 ? ((cls >= 2 && pp >= b2) ? 2 : 1) : 0;
                const u32 lo = j == 0 ? lo_[0] : (j == 1 ? lo_[1] : lo_[2]);
                const u32 hi = j == 0 ? hi_[0] : (j == 1 ? hi_[1] : hi_[2]);
                const u32 kind = hi >> 30;
                const int se = i0 + j < SEG_CAP ? i0 + j : SEG_CAP - 1;
                if (kind == K_REF) { av4[i] = -1; ap4[i] = (int)(seg_delta(lo, hi) + pp - c_s); }
                else if (kind == K_ALLELE) { av4[i] = pl.s_a[se]; ap4[i] = pl.s_b[se]; }
                else { av4[i] = -1; ap4[i] = kind == K_PAD_LEAD ? -1 : 2147483647; }
            }
        }
        finish(p0, rdl(d_pc0, u), rdl(d_pcn, u), wv, av4, ap4);
    };
    u32 gmask, mmask, umask;
    {
        const u64 bg = __builtin_amdgcn_ballot_w64(lane < CHUNK_TRIPS && lo_clip + lane * TRIP < limit && d_cls == 3);
        const u64 bm = __builtin_amdgcn_ballot_w64(lane < CHUNK_TRIPS && lo_clip + lane * TRIP < limit && (d_cls == 1 || d_cls == 2));
        const u64 bu = __builtin_amdgcn_ballot_w64(lane < CHUNK_TRIPS && lo_clip + lane * TRIP < limit && d_cls == 0);
        gmask = (u32)bg; mmask = (u32)bm; umask = (u32)bu;
    }
    // the first two multi trips: loads now, finish after the class-0 loads are out
    int mu_a = -1, mu_b = -1;
    u32 wa[3] = {0, 0, 0}, wb[3] = {0, 0, 0};
    if (mmask) { mu_a = __builtin_ctz(mmask); mmask &= mmask - 1; multi_issue(mu_a, wa); }
    if (mmask) { mu_b = __builtin_ctz(mmask); mmask &= mmask - 1; multi_issue(mu_b, wb); }
    // pass A: class-0 trips, 4 bytes per lane from one scalar base (computed in P3b)
    {
        // trips whose speculative read is the one the plan asks for (lane u holds trip u's descriptor)
        const u64 want = ((u64)d_ldhi << 32) | d_ldlo;
        const u64 spec = (u64)(A.ref + (g_delta + lo_clip)) + (u64)(u32)(lane * TRIP);
        const u32 have = spmask & (u32)__builtin_amdgcn_ballot_w64(lane < CHUNK_TRIPS && d_cls == 0 && want == spec);
        const u32 todo = umask & ~have;
#pragma unroll
        for (int u = 0; u < CHUNK_TRIPS; ++u) {
            if ((todo >> u) & 1u) {
                const u8 *src = reinterpret_cast<const u8 *>(((u64)(u32)rdl((int)d_ldhi, u) << 32) | (u32)rdl((int)d_ldlo, u));
                wq[u] = 0;
                if (lane4 < limit - (lo_clip + u * TRIP) && !(A.dbg & GVL_ABL(DBG_ABL_NO_LOADS))) wq[u] = load_u32_unaligned(src + (u32)lane4);
            }
        }
    }
    if (mu_a >= 0) multi_finish(mu_a, wa);
    if (mu_b >= 0) multi_finish(mu_b, wb);
    while (mmask) {   // a third, fourth ... multi trip in one chunk: one at a time
        const int u = __builtin_ctz(mmask);
        mmask &= mmask - 1;
        u32 w3[3];
        multi_issue(u, w3);
        multi_finish(u, w3);
    }
    GVL_STAMP(6);
#ifdef GVL_DIAG
    if (A.stamps && tid == 0) A.stamps[((u64)blockIdx.x * gridDim.y + blockIdx.y) * 16 + 10] = __builtin_popcount(gmask);
#endif
    // pass G: general trips (a segment boundary / allele / pad / row end inside the trip).
    // A group of 4 bases overlaps at most 4 segments; each contributes one masked dword
    // load from ITS source, so the group costs one memory latency, not one per byte.
    while (gmask) {
        const int u = __builtin_ctz(gmask);
        gmask &= gmask - 1;
        const int p0 = lo_clip + u * TRIP;
        const int p = p0 + GROUP * lane;
        u32 wv = 0;
        int av4[GROUP], ap4[GROUP];
        if (ANNOT) {
#pragma unroll
            for (int i = 0; i < GROUP; ++i) { av4[i] = -1; ap4[i] = -1; }
        }
        if (p < limit) {
            // segment holding p: the trip's first segment + the starts before p (independent
            // LDS reads; a fifth boundary inside one trip falls through to the while loop)
            const int s0 = __builtin_amdgcn_readlane(d_idx, u);
            int seg = s0;
            {
                int c = 0;
#pragma unroll
                for (int j = 1; j <= 4; ++j) {
                    const int sj = s0 + j < SEG_CAP ? s0 + j : SEG_CAP - 1;
                    c += (s0 + j < nseg && pl.s_out[sj] <= p) ? 1 : 0;
                }
                seg += c;
                if (c == 4) while (seg + 1 < nseg && pl.s_out[seg + 1] <= p) ++seg;
            }
            const int g_end = (limit - p > GROUP) ? p + GROUP : limit;
            // table entries seg .. seg+3 (a group of 4 bases overlaps at most 4 segments)
            u32 e_lo[GROUP], e_hi[GROUP]; int e_nx[GROUP];
#pragma unroll
            for (int t = 0; t < GROUP; ++t) {
                const int st = seg + t < SEG_CAP ? seg + t : SEG_CAP - 1;
                const int sn = seg + t + 1 < SEG_CAP ? seg + t + 1 : SEG_CAP - 1;
                e_lo[t] = pl.s_lo[st]; e_hi[t] = pl.s_hi[st];
                e_nx[t] = seg + t + 1 < nseg ? pl.s_out[sn] : limit;
            }
            int cur = p;
            u32 words[GROUP], masks[GROUP];
#pragma unroll
            for (int t = 0; t < GROUP; ++t) {
                words[t] = 0; masks[t] = 0;
                if (cur < g_end) {
                    const u32 lo = e_lo[t], hi = e_hi[t];
                    const u32 kind = hi >> 30;
                    const int s_end = e_nx[t];
                    const int e = s_end < g_end ? s_end : g_end;
                    const u32 m_hi = (e - p) >= 4 ? 0xFFFFFFFFu : ((1u << (8 * (e - p))) - 1u);
                    const u32 m_lo = (1u << (8 * (cur - p))) - 1u;
                    masks[t] = m_hi & ~m_lo;
                    const i64 src = seg_delta(lo, hi) + p;
                    if (ref_zero_fill) {
                        words[t] = 0;
                    } else if (kind == K_REF || kind == K_ALLELE) {
                        const u8 *arr = kind == K_REF ? A.ref : A.alt_alleles;
                        const i64 alen_ = kind == K_REF ? A.ref_len : A.alt_len;
                        if (src >= 0 && src + GROUP <= alen_) {
                            words[t] = load_u32_unaligned(arr + src);
                        } else {   // array edge: byte by byte, out of range -> pad
                            u32 wb = 0;
#pragma unroll
                            for (int i = 0; i < GROUP; ++i) {
                                const i64 s2 = src + i;
                                const u32 bb = (p + i >= cur && p + i < e && s2 >= 0 && s2 < alen_) ? (u32)arr[s2] : padb;
                                wb |= bb << (8 * i);
                            }
                            words[t] = wb;
                        }
                    } else {
                        words[t] = padb * 0x01010101u;
                    }
                    if (ANNOT) {
                        const int st = seg + t < SEG_CAP ? seg + t : SEG_CAP - 1;
#pragma unroll
                        for (int i = 0; i < GROUP; ++i) {
                            if (p + i >= cur && p + i < e) {
                                if (kind == K_REF) { av4[i] = -1; ap4[i] = (int)(src - c_s) + i; }
                                else if (kind == K_ALLELE) { av4[i] = pl.s_a[st]; ap4[i] = pl.s_b[st]; }
                                else { av4[i] = -1; ap4[i] = kind == K_PAD_LEAD ? -1 : 2147483647; }
                            }
                        }
                    }
                    cur = e;
                }
            }
#pragma unroll
            for (int t = 0; t < GROUP; ++t) wv |= words[t] & masks[t];
        }
        wv = finish(p0, rdl(d_pc0, u), rdl(d_pcn, u), wv, av4, ap4);
        finish_partial(p0, wv, av4, ap4);
    }
    GVL_STAMP(7);
    __builtin_amdgcn_s_setprio(0);
    // pass B: finish the class-0 trips.  Store addresses are a scalar base per trip plus a
    // per-lane offset that never changes: forward rows put lane l at +16*l, reverse-complemented
    // rows mirror the index (lane l at +16*(63-l) from the trip's lowest address).
    {
        const int jo_base = rc ? (L - GROUP - lo_clip - GROUP * (WAVE - 1)) : lo_clip;
        const int jo_step = rc ? -TRIP : TRIP;
        const u32 lane_rev = rc ? (u32)(WAVE - 1 - lane) : (u32)lane;
#pragma unroll
        for (int u = 0; u < CHUNK_TRIPS; ++u) {
            if ((umask >> u) & 1u) {
                const int p0 = lo_clip + u * TRIP;
                const int pc0 = rdl(d_pc0, u), pcn = rdl(d_pcn, u);
                u32 wv = wq[u];
                int av4[GROUP], ap4[GROUP];
                if (ANNOT) {
                    const u32 lo = (u32)rdl((int)d_lo0, u), hi = (u32)rdl((int)d_hi0, u);
                    const u32 kind = hi >> 30;
                    const int se = rdl(d_idx, u);
#pragma unroll
                    for (int i = 0; i < GROUP; ++i) {
                        if (kind == K_REF) { av4[i] = -1; ap4[i] = (int)(seg_delta(lo, hi) + p0 + lane4 + i - c_s); }
                        else { av4[i] = pl.s_a[se]; ap4[i] = pl.s_b[se]; }
                    }
                }
                for (int q = pc0; q < pcn; ++q) {
                    const u32 dd = (u32)(pl.p_out[q] - p0 - lane4);
                    if (dd < (u32)GROUP) {
                        const u32 sh = dd * 8;
                        wv = (wv & ~(0xFFu << sh)) | ((u32)pl.p_val[q] << sh);
                    }
                    if (ANNOT) {
                        const int pid = pl.p_id[q];
#pragma unroll
                        for (int i = 0; i < GROUP; ++i) if (dd == (u32)i) av4[i] = pid;
                    }
                }
                if (lane4 < limit - p0 && !(A.dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
                    const i64 jo0 = (i64)(jo_base + u * jo_step);       // scalar
                    const u32 ww = __builtin_amdgcn_perm(0u, wv, rc_sel);
                    const u32 b0_ = ww & 0xFF, b1_ = (ww >> 8) & 0xFF, b2_ = (ww >> 16) & 0xFF, b3_ = ww >> 24;
                    if (OH == OH_LC) {
                        u32x4_a4 o = {oh_t[b0_], oh_t[b1_], oh_t[b2_], oh_t[b3_]};
                        store_oh16(oh_row + 4 * jo0 + 16u * lane_rev, o);
                    } else if (OH == OH_CL) {
                        const u32 d0 = oh_t[b0_], d1 = oh_t[b1_], d2 = oh_t[b2_], d3 = oh_t[b3_];
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            const u32 sh = 8 * a;
                            const u32 v = ((d0 >> sh) & 0xFF) | (((d1 >> sh) & 0xFF) << 8) |
                                          (((d2 >> sh) & 0xFF) << 16) | (((d3 >> sh) & 0xFF) << 24);
                            store_u32_unaligned(oh_row + (i64)a * L + jo0 + 4u * lane_rev, v);
                        }
                    }
                    if (HAPS) {
                        u32 hv = ww;
                        if (rc) hv = (u32)luts.comp[b0_] | ((u32)luts.comp[b1_] << 8) | ((u32)luts.comp[b2_] << 16) | ((u32)luts.comp[b3_] << 24);
                        store_u32_unaligned(hap_row + jo0 + 4u * lane_rev, hv);
                    }
                    if (ANNOT) {
                        if (av_row) {
                            i32x4_a4 o = rc ? i32x4_a4{av4[3], av4[2], av4[1], av4[0]} : i32x4_a4{av4[0], av4[1], av4[2], av4[3]};
                            store_i32x4(av_row + jo0 + 4u * lane_rev, o.x, o.y, o.z, o.w);
                        }
                        if (ap_row) {
                            i32x4_a4 o = rc ? i32x4_a4{ap4[3], ap4[2], ap4[1], ap4[0]} : i32x4_a4{ap4[0], ap4[1], ap4[2], ap4[3]};
                            store_i32x4(ap_row + jo0 + 4u * lane_rev, o.x, o.y, o.z, o.w);
                        }
                    }
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    GVL_STAMP(8);
#ifdef GVL_DIAG
    if (A.stamps && lane == 0) {   // every wave: latest / earliest end of the workgroup
        unsigned long long *b = (unsigned long long *)&A.stamps[((u64)blockIdx.x * gridDim.y + blockIdx.y) * 16];
        const unsigned long long t = __builtin_amdgcn_s_memrealtime();
        atomicMax(b + 11, t);
        atomicMin(b + 12, t);
    }
#endif
}

#undef GVL_STAMP

