// gvl_diffs.inc -- length deltas (get_diffs_sparse), offsets scans, scratch-track and ragged-row sizing: device functions and
// kernels (included inside the including file's anonymous namespace, behind gvl_dev.inc).

// ---------------------------------------------------------------------------
// get_diffs_sparse (genotypes/mod.rs:15-125): one lane per (query, hap) row.
// ---------------------------------------------------------------------------

// length delta of one haplotype (genotype slot o_idx; keep slice at ks; optional query window)
__device__ __forceinline__ i64 row_diff_core(const DiffArgs &A, const i64 o_idx, const bool has_keep, const i64 ks,
                                             const bool has_query, const i64 q_start, const i64 q_end) {
    const i64 o_s = A.go_starts[o_idx], o_e = A.go_stops[o_idx];
    i64 acc = 0;
    if (o_e - o_s <= 0) return 0;
    if (has_query) {                                               // mod.rs:48-85
        i64 ref_idx = q_start;
        for (i64 v = o_s; v < o_e; ++v) {
            if (has_keep && !A.keep[ks + (v - o_s)]) continue;
            i64 vs, il;
            if (A.grec) {
                const int2 r = *reinterpret_cast<const int2 *>(A.grec + v);
                vs = r.x; il = r.y;
            } else {
                const i64 vi = A.geno_v_idxs[v];
                vs = A.v_starts[vi];
                il = A.ilens[vi];
            }
            const i64 v_end = vs - imin(il, 0) + 1;
            if (v_end <= q_start) continue;
            if (vs >= q_end) break;
            if (vs >= q_start && vs < ref_idx) continue;
            ref_idx = imax(ref_idx, v_end);
            if (il < 0) il += imax(q_start - vs - 1, 0);
            il += imax(v_end - q_end, 0);
            acc += il;
        }
    } else {                                                       // mod.rs:86-103
        for (i64 v = o_s; v < o_e; ++v) {
            if (has_keep && !A.keep[ks + (v - o_s)]) continue;
            acc += A.grec ? (i64)A.grec[v].ilen : (i64)A.ilens[A.geno_v_idxs[v]];
        }
    }
    return acc;
}

// The same, one WAVE per haplotype, 64 variants per trip (one coalesced read of the records).  The
// walk is sequential only through "skip a variant that starts inside what an applied variant already
// covers" (mod.rs:70): variant i is applied iff NOT (q_start <= pos_i < max(q_start, v_end of every
// applied variant before it)) -- an exclusive prefix-max over the applied set, iterated to its fixed
// point (unique: membership of i depends on the applied set in front of i only; each round settles at
// least one more lane).  The break at the first pos >= q_end is a filter because positions are sorted.
__device__ __forceinline__ i64 wave_excl_prefix_max64(i64 x, const int lane) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const i64 y = __shfl_up(x, o, WAVE);
        if (lane >= o) x = imax(x, y);
    }
    const i64 p = __shfl_up(x, 1, WAVE);
    return lane == 0 ? (i64)(-0x7FFFFFFFFFFFFFFFll - 1) : p;
}
__device__ __forceinline__ i64 row_diff_wave(const DiffArgs &A, const i64 o_idx, const bool has_keep, const i64 ks,
                                              const bool has_query, const i64 q_start, const i64 q_end, const int lane) {
    const i64 o_s = rfl64(A.go_starts[o_idx]), o_e = rfl64(A.go_stops[o_idx]);
    i64 acc = 0, carry = q_start;
    for (i64 b = o_s; b < o_e; b += WAVE) {
        const i64 v = b + lane;
        i64 vs = 0, il = 0;
        bool valid = v < o_e;
        if (valid) {
            if (A.grec) {
                const int2 r = *reinterpret_cast<const int2 *>(A.grec + v);
                vs = r.x; il = r.y;
            } else {
                const i64 vi = A.geno_v_idxs[v];
                il = A.ilens[vi];
                if (has_query) vs = A.v_starts[vi];
            }
            if (has_keep) valid = A.keep[ks + (v - o_s)] != 0;
        }
        i64 x = 0;
        if (!has_query) {                                          // mod.rs:86-103: a (masked) sum
            x = valid ? il : 0;
        } else {                                                   // mod.rs:48-85
            const i64 v_end = vs - imin(il, 0) + 1;
            const bool cand = valid && v_end > q_start && vs < q_end;
            bool inB = cand;
            u64 mB = __builtin_amdgcn_ballot_w64(inB);
            for (int it = 0; it < WAVE + 1; ++it) {
                i64 pm = wave_excl_prefix_max64(inB ? v_end : (i64)(-0x7FFFFFFFFFFFFFFFll - 1), lane);
                pm = imax(pm, carry);
                inB = cand && !(vs >= q_start && vs < pm);
                const u64 m2 = __builtin_amdgcn_ballot_w64(inB);
                if (m2 == mB) break;
                mB = m2;
            }
            if (inB) {
                i64 d = il;
                if (d < 0) d += imax(q_start - vs - 1, 0);
                d += imax(v_end - q_end, 0);
                x = d;
            }
            i64 mx = inB ? v_end : carry;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = imax(mx, __shfl_xor(mx, o, WAVE));
            carry = imax(carry, mx);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, WAVE);
        acc += x;
        if (has_query && __builtin_amdgcn_ballot_w64(v < o_e && vs >= q_end) != 0) break;   // sorted: nothing further counts
    }
    return acc;
}

__device__ __forceinline__ i64 row_diff(const DiffArgs &A, i64 k) {
    const i64 query = k / A.ploidy;
    const bool has_query = A.q_starts && A.q_ends && A.v_starts;   // mod.rs:35
    const bool has_keep = A.keep && A.keep_offsets;                // mod.rs:36
    const i64 ks = has_keep ? A.keep_offsets[k] : 0;
    const i64 q_start = has_query ? (i64)A.q_starts[query * A.q_stride] : 0;
    const i64 q_end = has_query ? (i64)A.q_ends[query * A.q_stride] : 0;
    return row_diff_core(A, A.geno_offset_idx[k], has_keep, ks, has_query, q_start, q_end);
}

__global__ __launch_bounds__(256) void diffs_kernel(const DiffArgs A, const int *regions,
                                                     i64 regions_stride) {
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n_rows) return;
    const int d = (int)row_diff(A, k);      // `as i32` truncation
    if (A.diffs) A.diffs[k] = d;
    if (A.lengths) {
        i64 len;
        if (A.output_length >= 0) {
            len = A.output_length;
        } else {
            const int *reg = regions + (k / A.ploidy) * regions_stride;
            len = imax((i64)(reg[2] - reg[1]) + d, 0);
        }
        if (A.len_cap > 0 && len > A.len_cap) { len = A.len_cap; if (A.async_err) *A.async_err = 1; }
        A.lengths[k + 1] = len;
        if (k == 0) A.lengths[0] = 0;
    }
}

__global__ __launch_bounds__(256) void diffs_wave_kernel(const DiffArgs A, const int *regions, i64 regions_stride) {
    const int lane = threadIdx.x & (WAVE - 1);
    const i64 k = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (k >= A.n_rows) return;
    const i64 query = k / A.ploidy;
    const bool has_query = A.q_starts && A.q_ends && A.v_starts;
    const bool has_keep = A.keep && A.keep_offsets;
    const i64 ks = has_keep ? rfl64(A.keep_offsets[k]) : 0;
    const i64 q_start = has_query ? (i64)rfl(A.q_starts[query * A.q_stride]) : 0;
    const i64 q_end = has_query ? (i64)rfl(A.q_ends[query * A.q_stride]) : 0;
    const int d = (int)row_diff_wave(A, rfl64(A.geno_offset_idx[k]), has_keep, ks, has_query, q_start, q_end, lane);
    if (lane != 0) return;
    if (A.diffs) A.diffs[k] = d;
    if (A.lengths) {
        i64 len;
        if (A.output_length >= 0) {
            len = A.output_length;
        } else {
            const int *reg = regions + query * regions_stride;
            len = imax((i64)(reg[2] - reg[1]) + d, 0);
        }
        if (A.len_cap > 0 && len > A.len_cap) { len = A.len_cap; if (A.async_err) *A.async_err = 1; }
        A.lengths[k + 1] = len;
        if (k == 0) A.lengths[0] = 0;
    }
}

// In-place inclusive scan of lengths[1..n] (lengths[0] = 0) by ONE workgroup;
// also reports {total, max}.  n is the batch's row count (thousands), so a single
// 1024-thread workgroup streaming the array is enough and keeps it one launch.
__global__ __launch_bounds__(1024) void offsets_scan_kernel(i64 *offs, i64 n, i64 *total_and_max) {
    __shared__ i64 wsum[16];
    __shared__ i64 wmax[16];
    __shared__ i64 carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    i64 mx = 0;
    for (i64 base = 0; base < n; base += 1024) {
        const i64 i = base + tid;
        i64 x = i < n ? offs[i + 1] : 0;
        mx = imax(mx, x);
        i64 s = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const i64 y = __shfl_up(s, o, 64);
            if (lane >= o) s += y;
        }
        if (lane == 63) wsum[wv] = s;
        __syncthreads();
        i64 pre = carry_s;
        for (int w = 0; w < wv; ++w) pre += wsum[w];
        if (i < n) offs[i + 1] = s + pre;
        __syncthreads();
        if (tid == 1023) carry_s = s + pre;
        __syncthreads();
    }
    if (total_and_max) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = imax(mx, __shfl_down(mx, o, 64));
        if (lane == 0) wmax[wv] = mx;
        __syncthreads();
        if (tid == 0) {
            i64 m = 0;
            for (int w = 0; w < 16; ++w) m = imax(m, wmax[w]);
            total_and_max[0] = carry_s;
            total_and_max[1] = m;
        }
    }
}

// Scratch-track lengths of a haps + tracks batch (_reconstruct.py:191): per query,
// len - min over haplotypes of min(diff, 0) with diff = the haplotype's length delta inside the
// window (query mode of get_diffs_sparse); written at lengths[q + 1] for the scan.  Also the
// (batch * ploidy + 1) fixed-length output offsets k * L that the realign kernel reads (ROW_OFFS).  Ragged rows (!ROW_OFFS): the
// caller's offsets (caller_offsets, never written) clamped to [0, batch * ploidy * len_cap] into out_offsets, which the realignment then
// reads -- nothing lands past a track's capacity -- and a row longer than A.len_cap or outside that capacity is reported through
// A.async_err.
// `pairs` != 0: lengths as (0, length) PAIRS per query -- what the realignment straight from the intervals needs (only differences of
// the offsets are read there: no scratch track, so no prefix sum and no scan launch).
// Ploidy 1 / 2 / 4 (round 6): a wave per (query, HAPLOTYPE) -- the haplotypes of a query share a workgroup and meet in LDS -- instead
// of one wave walking the query's haplotypes one after the other (12 us of a stand-alone gvl_tracks_batch for 128 queries of 170
// variants per haplotype).
template <bool ROW_OFFS>
__global__ __launch_bounds__(256) void track_lengths_kernel(const DiffArgs A, const int *regions, i64 regions_stride, i64 batch,
                                                             i64 out_len, i64 *lengths, i64 *out_offsets, int pairs, const i64 *caller_offsets) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 K = batch * A.ploidy;
    if constexpr (ROW_OFFS) {
        for (i64 k = t; k <= K; k += (i64)gridDim.x * blockDim.x) out_offsets[k] = k * out_len;
    } else {
        const i64 cap = K * A.len_cap;
        for (i64 k = t; k <= K; k += (i64)gridDim.x * blockDim.x) {
            const i64 o0 = caller_offsets[k];
            out_offsets[k] = o0 < 0 ? 0 : (o0 > cap ? cap : o0);
            if (k < K) {
                const i64 o1 = caller_offsets[k + 1];
                if ((o0 < 0 || o1 < o0 || o1 - o0 > A.len_cap || o1 > cap) && A.async_err) atomicOr(A.async_err, 1);
            }
        }
    }
    const int lane = threadIdx.x & (WAVE - 1);
    auto put = [&](const i64 q, const i64 len) {
        if (pairs) { lengths[2 * q] = 0; lengths[2 * q + 1] = len; }
        else { lengths[q + 1] = len; if (q == 0) lengths[0] = 0; }
    };
    if (A.ploidy == 1 || A.ploidy == 2 || A.ploidy == 4) {
        __shared__ int s_mn[4];
        const int wave = (int)(threadIdx.x >> 6);
        const int per_wg = 4 / A.ploidy;                         // queries of this workgroup
        const int qi = wave / A.ploidy, p = wave - qi * A.ploidy;
        const i64 q = (i64)blockIdx.x * per_wg + qi;
        if (threadIdx.x < 4) s_mn[threadIdx.x] = 0;
        __syncthreads();
        i64 qs = 0, qe = 0;
        if (q < batch) {
            const int *reg = regions + q * regions_stride;
            qs = rfl(reg[1]); qe = rfl(reg[2]);
            const int d = (int)row_diff_wave(A, rfl64(A.geno_offset_idx[q * A.ploidy + p]), false, 0, true, qs, qe, lane);
            if (lane == 0 && d < 0) atomicMin(&s_mn[qi], d);
        }
        __syncthreads();
        if (q < batch && p == 0 && lane == 0) put(q, (qe - qs) - (i64)s_mn[qi]);
        return;
    }
    const i64 q = t >> 6;                                    // one wave per query
    if (q >= batch) return;
    const int *reg = regions + q * regions_stride;
    const i64 qs = rfl(reg[1]), qe = rfl(reg[2]);
    i64 mn = 0;
    for (int p = 0; p < A.ploidy; ++p) {
        const i64 d = (i64)(int)row_diff_wave(A, rfl64(A.geno_offset_idx[q * A.ploidy + p]), false, 0, true, qs, qe, lane);
        mn = d < mn ? d : mn;
    }
    if (lane == 0) put(q, (qe - qs) - mn);
}

// The same for every query of an EPOCH (gvl_loader_start_epoch: the jittered regions and the length deltas of
// every query are known there), laid out per batch: batch j's (bs + 1) scan slots at lengths[j * (bs + 1) ..],
// slot 0 = 0; track_scan_batches_kernel then turns each batch's slots into its scratch-track offsets.  A batch
// of the epoch then costs no sizing launch at all (they were 19 us of cfg4's 143 us step).
template <bool ROW_OFFS>
__global__ __launch_bounds__(256) void track_lengths_epoch_kernel(const DiffArgs A, const int *regions, i64 regions_stride, i64 n,
                                                                   i64 bs, i64 out_len, i64 *lengths, i64 *out_offsets) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 K = bs * A.ploidy;
    if constexpr (ROW_OFFS)
        for (i64 k = t; k <= K; k += (i64)gridDim.x * blockDim.x) out_offsets[k] = k * out_len;
    const int lane = threadIdx.x & (WAVE - 1);
    const i64 q = t >> 6;                                    // one wave per query
    if (q >= n) return;
    const int *reg = regions + q * regions_stride;
    const i64 qs = rfl(reg[1]), qe = rfl(reg[2]);
    i64 mn = 0;
    for (int p = 0; p < A.ploidy; ++p) {
        const i64 d = (i64)(int)row_diff_wave(A, rfl64(A.geno_offset_idx[q * A.ploidy + p]), false, 0, true, qs, qe, lane);
        mn = d < mn ? d : mn;
    }
    if (lane == 0) {
        const i64 j = q / bs, i = q - j * bs;
        lengths[j * (bs + 1) + i + 1] = (qe - qs) - mn;
        if (i == 0) lengths[j * (bs + 1)] = 0;
    }
}
// one workgroup per batch: inclusive scan of its (bs + 1) slots in place (slot 0 is 0, so slot i = offset of query i)
__global__ __launch_bounds__(256) void track_scan_batches_kernel(i64 *lengths, i64 n, i64 bs) {
    __shared__ i64 wsum[4];
    __shared__ i64 carry_s;
    const i64 j = blockIdx.x;
    const i64 cnt = (n - j * bs < bs ? n - j * bs : bs) + 1;
    i64 *a = lengths + j * (bs + 1);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (i64 base = 0; base < cnt; base += 256) {
        const i64 i = base + tid;
        i64 sc = i < cnt ? a[i] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const i64 y = __shfl_up(sc, o, 64);
            if (lane >= o) sc += y;
        }
        if (lane == 63) wsum[wv] = sc;
        __syncthreads();
        i64 pre = carry_s;
        for (int w = 0; w < wv; ++w) pre += wsum[w];
        if (i < cnt) a[i] = sc + pre;
        __syncthreads();
        if (tid == 255) carry_s = sc + pre;
        __syncthreads();
    }
}

// The ragged sizing of a whole GROUP of batches in two launches (the native loader's ragged groups; per batch it was two
// latency-bound launches each, 16 us per batch alone -- twice the reconstruct grid's time).  The group's request arrays are
// consecutive rows of the epoch table, its offsets live in the batches' own slots: a pointer per batch in the kernarg segment.
struct HapGroupOut { i64 *offs[GVL_MANY_MAX]; i64 *sizes[GVL_MANY_MAX]; };
__global__ __launch_bounds__(256) void hap_lengths_group_kernel(const DiffArgs A, const int *regions, i64 regions_stride, i64 rows_per_batch,
                                                                 const HapGroupOut O) {
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n_rows) return;
    const int d = (int)row_diff(A, k);      // `as i32` truncation
    const int *reg = regions + (k / A.ploidy) * regions_stride;
    i64 len = imax((i64)(reg[2] - reg[1]) + d, 0);                  // src/ffi/mod.rs:801-807
    if (A.len_cap > 0 && len > A.len_cap) { len = A.len_cap; if (A.async_err) *A.async_err = 1; }
    const i64 b = k / rows_per_batch, i = k - b * rows_per_batch;
    i64 *const offs = O.offs[b];
    offs[i + 1] = len;
    if (i == 0) offs[0] = 0;
}
// one workgroup per batch: the row lengths at offs[1 ..] become offsets in place; sizes = {total, longest row}
__global__ __launch_bounds__(256) void hap_scan_group_kernel(const HapGroupOut O, i64 rows_per_batch, i64 n_rows_total) {
    __shared__ i64 wsum[4];
    __shared__ i64 wmax[4];
    __shared__ i64 carry_s;
    const i64 j = blockIdx.x;
    const i64 n = (n_rows_total - j * rows_per_batch < rows_per_batch) ? n_rows_total - j * rows_per_batch : rows_per_batch;
    i64 *const offs = O.offs[j];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    i64 mx = 0;
    for (i64 base = 0; base < n; base += 256) {
        const i64 i = base + tid;
        const i64 x = i < n ? offs[i + 1] : 0;
        mx = imax(mx, x);
        i64 sc = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const i64 y = __shfl_up(sc, o, 64);
            if (lane >= o) sc += y;
        }
        if (lane == 63) wsum[wv] = sc;
        __syncthreads();
        i64 pre = carry_s;
        for (int w = 0; w < wv; ++w) pre += wsum[w];
        if (i < n) offs[i + 1] = sc + pre;
        __syncthreads();
        if (tid == 255) carry_s = sc + pre;
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = imax(mx, __shfl_down(mx, o, 64));
    if (lane == 0) wmax[wv] = mx;
    __syncthreads();
    if (tid == 0 && O.sizes[j]) {
        O.sizes[j][0] = carry_s;
        O.sizes[j][1] = imax(imax(wmax[0], wmax[1]), imax(wmax[2], wmax[3]));
    }
}

// The same sizing for EVERY batch of an epoch at once (the native loader's table, filled once per epoch and a whole epoch ahead):
// batch j's offsets at offs_base + j * (rows_per_batch + 1), its {total, longest row} at sizes_base + 2 j.  A group's launch then
// reads its rows' offsets from the table -- no sizing pass in front of it -- and a copy kernel BEHIND it hands them to the
// consumer's slots.
__global__ __launch_bounds__(256) void hap_lengths_epoch_kernel(const DiffArgs A, const int *regions, i64 regions_stride, i64 rows_per_batch,
                                                                 i64 *offs_base) {
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n_rows) return;
    const int d = (int)row_diff(A, k);      // `as i32` truncation
    const int *reg = regions + (k / A.ploidy) * regions_stride;
    i64 len = imax((i64)(reg[2] - reg[1]) + d, 0);                  // src/ffi/mod.rs:801-807
    if (A.len_cap > 0 && len > A.len_cap) { len = A.len_cap; if (A.async_err) *A.async_err = 1; }
    const i64 b = k / rows_per_batch, i = k - b * rows_per_batch;
    i64 *const offs = offs_base + b * (rows_per_batch + 1);
    offs[i + 1] = len;
    if (i == 0) offs[0] = 0;
}
__global__ __launch_bounds__(256) void hap_scan_epoch_kernel(i64 *offs_base, i64 *sizes_base, i64 rows_per_batch, i64 n_rows_total) {
    __shared__ i64 wsum[4];
    __shared__ i64 wmax[4];
    __shared__ i64 carry_s;
    const i64 j = blockIdx.x;
    const i64 n = (n_rows_total - j * rows_per_batch < rows_per_batch) ? n_rows_total - j * rows_per_batch : rows_per_batch;
    i64 *const offs = offs_base + j * (rows_per_batch + 1);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    i64 mx = 0;
    for (i64 base = 0; base < n; base += 256) {
        const i64 i = base + tid;
        const i64 x = i < n ? offs[i + 1] : 0;
        mx = imax(mx, x);
        i64 sc = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const i64 y = __shfl_up(sc, o, 64);
            if (lane >= o) sc += y;
        }
        if (lane == 63) wsum[wv] = sc;
        __syncthreads();
        i64 pre = carry_s;
        for (int w = 0; w < wv; ++w) pre += wsum[w];
        if (i < n) offs[i + 1] = sc + pre;
        __syncthreads();
        if (tid == 255) carry_s = sc + pre;
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = imax(mx, __shfl_down(mx, o, 64));
    if (lane == 0) wmax[wv] = mx;
    __syncthreads();
    if (tid == 0) {
        sizes_base[2 * j] = carry_s;
        sizes_base[2 * j + 1] = imax(imax(wmax[0], wmax[1]), imax(wmax[2], wmax[3]));
    }
}
// a group's offsets and sizes from the table to its batches' slots (blockIdx.y = batch of the group)
__global__ __launch_bounds__(256) void hap_offsets_copy_kernel(const HapGroupOut O, const i64 *offs_src, const i64 *sizes_src, i64 rows_per_batch) {
    const int b = blockIdx.y;
    const i64 *const src = offs_src + (i64)b * (rows_per_batch + 1);
    i64 *const dst = O.offs[b];
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i <= rows_per_batch; i += (i64)gridDim.x * blockDim.x) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x < 2 && O.sizes[b]) O.sizes[b][threadIdx.x] = sizes_src[2 * b + threadIdx.x];
}
