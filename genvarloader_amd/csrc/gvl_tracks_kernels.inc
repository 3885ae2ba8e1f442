// gvl_tracks_kernels.inc -- track kernels (included inside gvl_tracks.hip's anonymous namespace, behind gvl_dev.inc + gvl_diffs.inc).

// ---------------------------------------------------------------------------------
// Tracks (SURVEY 8 row a12, BASELINE config 4): interval painting and realignment of
// reference-coordinate f32 tracks to a haplotype.  One wave per (row, chunk): the walk is
// planned with wave scans (lane j = variant j) into a 64-entry LDS table of the chunk's
// entries, then the wave streams 4 values per lane per trip; values inside a plain track run
// are one 16-B load + one 16-B store.  Rows the planner cannot express (coordinates beyond
// 2^30, > 64 entries per chunk) replay the reference's walk on the scalar unit with the same
// flush/compaction scheme as recon_wave_scalar.
// ---------------------------------------------------------------------------------
enum : int { T_TRACK = 0, T_REPEAT = 1, T_FILL = 2, T_ZERO = 3 };
struct TrackMirror { int out[SEG_CAP]; int kind[SEG_CAP]; int plo[SEG_CAP]; int phi[SEG_CAP]; int vlen[SEG_CAP]; };

// ---- where the realignment reads a query's reference-coordinate track from -------------------------------
// SrcGlobal: a track in memory (gvl_realign_tracks; the scratch track the painter wrote).
// SrcPainted: the query's INTERVALS -- src/intervals.rs:19-126 evaluated at the positions the realignment asks for,
// so that the scratch track is neither written nor read (BASELINE config 4: 67 MB each way per batch, and one
// launch).  Position x of the track = reference position qs + x; its value = that of the last interval (in order)
// that covers it, 0.0 if none.  The wave keeps a WINDOW of the track as the tiled painter keeps a chunk: the
// candidate intervals' values / ends and a bitmap of their starts with its popcount prefix -- for a position in
// the window two LDS reads give the only candidate that can cover it (non-overlapping candidates; a window whose
// candidates overlap, or more than PAINT_TILE of them, is not used).  Any other position is looked up in the
// list itself (binary search + walk back under the running maximum of ends, as the per-value painter does):
// exactness never depends on what the window holds.
constexpr int PAINT_TILE = 256;
constexpr int PAINT_CHUNK = 2048;
constexpr int PAINT_WIN = 4096;                 // window positions (a chunk's 2048 + what its deletions skip + slack)
struct PaintIndex { const i64 *offsets; const int *base; const int *lo; const int *hi; };
struct PaintSrcArgs {                           // the interval set of one track (gvl_track_set) for the kernel
    const i64 *offset_idxs; i64 list_div;
    const int *itv_starts; const int *itv_ends; const float *itv_values; const i64 *itv_offsets; const int *pmax;
    PaintIndex X;
};
// The window as BREAKPOINTS: a bit per position where the track's value changes -- an interval's start (to its value) or its end (to
// 0.0, unless the next interval starts right there) -- and the values behind the breakpoints in order, bv[0] = 0.0 = "in front of the
// first one".  The value at window position r is bv[breakpoints at or in front of r]: a popcount and ONE read, no end to compare
// with (round 4 kept candidates' values + ends and compared: 8 VALU per value; gaps as zero-valued entries: 4).
struct PaintWin { u32 bm[PAINT_WIN / 32 + 2]; u32 pre[PAINT_WIN / 32]; float bv[2 * PAINT_TILE + 2]; };   // (+ zero words behind the bitmap)

struct SrcGlobal {
    const float *track; i64 tlen;
    __device__ __forceinline__ float at(const i64 x) const { return (x >= 0 && x < tlen) ? track[x] : 0.0f; }
    // (0 <= x, x + 4 <= tlen)
    __device__ __forceinline__ void at4(const i64 x, float (&v)[4]) const {
        const float *src = track + x;
        v[0] = src[0]; v[1] = src[1]; v[2] = src[2]; v[3] = src[3];
    }
    __device__ __forceinline__ void at4i(const int x, float (&v)[4]) const { at4((i64)x, v); }
    __device__ __forceinline__ void at8i(const int x, float (&v)[8]) const {
        const float *src = track + x;
#pragma unroll
        for (int g = 0; g < 8; ++g) v[g] = src[g];
    }
    template <int N> __device__ __forceinline__ void winN(const int, float (&)[N]) const {}
    __device__ __forceinline__ bool covers(const i64, const i64) const { return false; }
    i64 x_lo = 0;
};
// One position looked up in the query's interval list itself (intervals.rs:19-126 for one position): binary search for the
// last start at or in front of it, then back under the running maximum of ends.  A real call, and the list's arrays
// are re-read from the kernel's arguments (`ps_kernarg` = where PaintSrcArgs sits in the kernarg segment): this is
// the rare path, and inlined it kept eight more pointers alive on the scalar side through the whole emit loop (the
// kernel spills scalars into vector lanes as it is: every such value costs a v_readlane where it is used).
typedef const PaintSrcArgs __attribute__((address_space(4))) *PaintSrcArgsK;
__device__ __noinline__ float paint_list_value(const u64 ps_kernarg, const i64 idx, const i64 qs, const i64 j) {
#if defined(__HIP_DEVICE_COMPILE__)
    const PaintSrcArgsK ps = (PaintSrcArgsK)(u64)rfl64((i64)ps_kernarg);
    const int *itv_starts = ps->itv_starts, *itv_ends = ps->itv_ends, *pmax = ps->pmax;
    const float *itv_values = ps->itv_values;
    const i64 li = rfl64(idx);
    const i64 s0 = ps->itv_offsets[li], e0 = ps->itv_offsets[li + 1];
    i64 lo = s0, hi = e0;                                      // first interval with start - qs > j
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if ((i64)itv_starts[mid] - qs <= j) lo = mid + 1; else hi = mid;
    }
    if (lo > s0 && (i64)pmax[lo - 1] - qs > j)
        for (i64 c = lo - 1; c >= s0; --c)
            if ((i64)itv_ends[c] - qs > j) return itv_values[c];
#endif
    return 0.0f;
}

struct SrcPainted {
    const PaintWin *W; i64 x_lo; int wlen; bool win_ok;
    i64 tlen, qs, idx;
    u64 ps_kernarg;
    u64 *stamps;
    __device__ __forceinline__ float in_win(const int r) const {
        const u32 wd = W->bm[r >> 5];
        return W->bv[(int)W->pre[r >> 5] + __builtin_popcount(wd & (0xFFFFFFFFu >> (31 - (r & 31))))];
    }
    __device__ __forceinline__ float in_list(const i64 j) const {
        if (stamps) atomicAdd((unsigned long long *)&stamps[14], 1ull);             // positions looked up in the list itself
        return paint_list_value(ps_kernarg, idx, qs, j);
    }
    __device__ __forceinline__ float at(const i64 x) const {
        if (x < 0 || x >= tlen) return 0.0f;
        const i64 r = x - x_lo;
        if (win_ok && r >= 0 && r < wlen) return in_win((int)r);
        return in_list(x);
    }
    // N consecutive window positions r .. r + N - 1 (N <= 8; inside the window): the breakpoints at or in front of r from the
    // bitmap's prefix + the word that holds r's bit and the one behind it as ONE 64-bit word (no special case for a group that
    // straddles two words), then per position the breakpoints between r and it -- a masked popcount with the count added -- and one read
    template <int N>
    __device__ __forceinline__ void winN(const int r, float (&v)[N]) const {
        const int bp = r & 31, wi = r >> 5;
        const u64 w = ((u64)W->bm[wi + 1] << 32) | W->bm[wi];
        const int c0 = (int)W->pre[wi] + __builtin_popcountll(w & (~0ull >> (63 - bp)));
        const u32 m = (u32)(w >> (bp + 1));               // bit g - 1: a breakpoint at position r + g
        v[0] = W->bv[c0];
#pragma unroll
        for (int g = 1; g < N; ++g) v[g] = W->bv[c0 + __builtin_popcount(m & ((1u << g) - 1u))];
    }
    // four consecutive positions (0 <= x, x + 4 <= tlen)
    __device__ __forceinline__ void at4(const i64 x, float (&v)[4]) const {
        const i64 r64 = x - x_lo;
        if (win_ok && r64 >= 0 && r64 + 4 <= wlen) { winN<4>((int)r64, v); return; }
#pragma unroll
        for (int g = 0; g < 4; ++g) v[g] = at(x + g);
    }
    // (positions below 2^31 - 8: the caller has checked the row's table and track length)
    __device__ __forceinline__ void at4i(const int x, float (&v)[4]) const {
        const int r = x - (int)x_lo;
        if (win_ok && r >= 0 && r + 4 <= wlen) { winN<4>(r, v); return; }
#pragma unroll
        for (int g = 0; g < 4; ++g) v[g] = at((i64)x + g);
    }
    __device__ __forceinline__ void at8i(const int x, float (&v)[8]) const {
        const int r = x - (int)x_lo;
        if (win_ok && r >= 0 && r + 8 <= wlen) { winN<8>(r, v); return; }
#pragma unroll
        for (int g = 0; g < 8; ++g) v[g] = at((i64)x + g);
    }
    // whether positions [x, x + n) all lie inside the window (then winN needs no test per group)
    __device__ __forceinline__ bool covers(const i64 x, const i64 n) const { return win_ok && x >= x_lo && x + n <= x_lo + wlen; }
};
__device__ __forceinline__ bool S_win_ok(const SrcPainted &S) { return S.win_ok; }
__device__ __forceinline__ bool S_win_ok(const SrcGlobal &) { return true; }
// One value of an insertion-fill region: src/tracks/mod.rs:87-190, evaluated per position.
// `i` = offset inside the region, `pp` = output index in the row.
template <class Src>
__device__ float fill_value(const TrackArgs &A, const Src &S, i64 vrp, i64 v_len, i64 i,
                            i64 pp, u64 query, u64 hap) {
#pragma clang fp contract(off)
    const i64 tlen = S.tlen;
    auto tr = [&](i64 x) -> float { return S.at(x); };
    if (A.strategy == GVL_FILL_REPEAT_5P) return tr(vrp);
    if (A.strategy == GVL_FILL_REPEAT_5P_NORM) return tr(vrp) / (float)v_len;
    if (A.strategy == GVL_FILL_CONSTANT) return (float)A.param;
    if (A.strategy == GVL_FILL_FLANK_SAMPLE) {
        const i64 width = (i64)A.param;
        const i64 lo = imax(vrp - width, 0), hi = imin(vrp + width, tlen - 1);
        const u64 pool = (u64)(hi - lo + 1);
        // (`query`: the batch row -- through the caller's map when one logical batch arrives in several calls, src/tracks/mod.rs:754-760)
        const u64 qseed = A.query_seed ? (u64)A.query_seed[query] : query;
        const u64 seed = hash4_dev(A.seed_ptr ? *A.seed_ptr : A.base_seed, qseed, hap, (u64)pp);
        return tr(lo + (i64)(pool ? seed % pool : 0));
    }
    if (A.strategy == GVL_FILL_INTERPOLATE) {
        const i64 order = (i64)A.param;
        const i64 k = (order + 1 + 1) / 2;
        const i64 n = 2 * k;
        auto xs = [&](i64 j) -> double { return j < k ? -(double)j : (double)v_len + (double)(j - k); };
        auto ys = [&](i64 j) -> double {
            return j < k ? (double)tr(imax(vrp - j, 0)) : (double)tr(imin(vrp + 1 + (j - k), tlen - 1));
        };
        const double x = (double)i;
        double acc = 0.0;
        for (i64 a = 0; a < n; ++a) {
            double term = ys(a);
            const double xa = xs(a);
            for (i64 b = 0; b < n; ++b) {
                if (b == a) continue;
                const double xb = xs(b);
                term = term * ((x - xb) / (xa - xb));
            }
            acc = acc + term;
        }
        return (float)acc;
    }
    return 0.0f;
}

// The window of a painted source (see PaintWin): from track position x_first - 64 on, at most PAINT_WIN positions.  -> false (nothing
// usable built) when the set has no bucket index, the window's buckets hold more than PAINT_TILE candidates, or the candidates overlap /
// share a start: positions are then looked up in the list itself.  PS = the interval set in the kernel's argument segment (its
// pointers are read HERE, not held on the scalar side since the kernel's start).
template <typename PSPtr>
__device__ __forceinline__ bool paint_build_window(PaintWin &Wn, const PSPtr PS, const i64 idx, const i64 q_start, const i64 tlen, const i64 x_first,
                                                   const int lane, i64 &x_lo_out, int &wlen_out) {
    i64 x_lo = x_first - 64;
    x_lo = x_lo < 0 ? 0 : x_lo;
    const i64 wl64 = tlen - x_lo;
    const int wlen = wl64 > PAINT_WIN ? PAINT_WIN : (wl64 < 0 ? 0 : (int)wl64);
    // (the interval set's pointers are read from the kernel's arguments HERE, not held on the scalar side since the
    // kernel's start: the walk in between needs every scalar register it can get)
    // the list's bounds and its bucket index's: four lanes of ONE load (+ the index's first position), then both bucket
    // bounds in one -- written value by value the compiler made each of them a memory round trip of its own, and the
    // kernel's time is the length of a wave's chain of dependent round trips as much as its instruction count
    // (measured: 59 us at 7 waves per SIMD, 67 at 4, 79 at 3)
    int h_lo = 0, h_hi = 0, h_b = 0;
    {
        const i64 *const io = PS->itv_offsets, *const xo = PS->X.offsets;
        const int *const xb = PS->X.base;
        if (lane < 4 && (lane < 2 || xo)) {
            const i64 h = lane < 2 ? io[idx + lane] : xo[idx + (lane - 2)];
            h_lo = (int)(u32)(u64)h; h_hi = (int)(u32)((u64)h >> 32);
        }
        if (lane == 0 && xb) h_b = xb[idx];
    }
    const i64 s0 = rdl64(h_lo, h_hi, 0), e0 = rdl64(h_lo, h_hi, 1);
    if (wlen <= 0 || !PS->X.offsets || e0 <= s0) return false;
    const i64 b0 = rdl64(h_lo, h_hi, 2);
    const i64 nb = rdl64(h_lo, h_hi, 3) - b0;
    if (nb <= 0) return false;
    const i64 bbase = rdl(h_b, 0);
    i64 ba = (q_start + x_lo - bbase) >> 11, bb = (q_start + x_lo + wlen - 1 - bbase) >> 11;
    ba = ba < 0 ? 0 : (ba > nb - 1 ? nb - 1 : ba);
    bb = bb < 0 ? 0 : (bb > nb - 1 ? nb - 1 : bb);
    int lohi = 0;
    if (lane < 2) lohi = lane == 0 ? PS->X.lo[b0 + ba] : PS->X.hi[b0 + bb];
    i64 lo_c = s0 + rdl(lohi, 0);
    const i64 hi_c = s0 + rdl(lohi, 1);
    if (lo_c > hi_c) lo_c = hi_c;
    if (hi_c - lo_c > PAINT_TILE) return false;
    const int n_c = (int)(hi_c - lo_c);
    Wn.bm[lane] = 0u; Wn.bm[WAVE + lane] = 0u;
    if (lane < 2) Wn.bm[2 * WAVE + lane] = 0u;
    if (lane == 0) Wn.bv[0] = 0.0f;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    bool bad = false;
    int carry_e = (int)0x80000000, carry_s = (int)0x80000000;          // end / start of the candidate in front
    // (all candidate records are requested before the first one is used: one memory round trip; rounds the
    // window has no candidates for are skipped as a whole)
    int c_s[PAINT_TILE / WAVE], c_e[PAINT_TILE / WAVE]; float c_v[PAINT_TILE / WAVE];
#pragma unroll
    for (int r_ = 0; r_ < PAINT_TILE / WAVE; ++r_) {
        const int i = r_ * WAVE + lane;
        c_s[r_] = 0; c_e[r_] = 0; c_v[r_] = 0.0f;
        if (r_ * WAVE < n_c) {
            if (i < n_c) { c_s[r_] = PS->itv_starts[lo_c + i]; c_e[r_] = PS->itv_ends[lo_c + i]; c_v[r_] = PS->itv_values[lo_c + i]; }
        }
    }
    const i64 qx64 = q_start + x_lo;             // the window's first position on the reference
    const bool qx_small = qx64 > -(1ll << 30) && qx64 < (1ll << 30);
    const int qx = (int)qx64;
    // pass 1: window-relative starts / ends (kept in c_s / c_e), the order check, the breakpoints' bits.  A candidate that ends at
    // or in front of the window's first position, or starts behind its last, sets nothing; the one that straddles the first
    // position (there is at most one: candidates do not overlap) starts AT it.
#pragma unroll
    for (int r_ = 0; r_ < PAINT_TILE / WAVE; ++r_) {
        const int b = r_ * WAVE;
        if (b >= n_c) break;
        const int i = b + lane;
        int sr = 0x7FFFFFFF, er = 0x7FFFFFFF;
        // 32-bit arithmetic when nothing can overflow it (always, for real coordinates), else 64-bit and clamped
        const bool small = qx_small && __builtin_amdgcn_ballot_w64(i < n_c && (c_s[r_] <= -(1 << 30) || c_s[r_] >= (1 << 30) ||
                                                                              c_e[r_] <= -(1 << 30) || c_e[r_] >= (1 << 30))) == 0;
        if (i < n_c) {
            if (small) {
                sr = c_s[r_] - qx; er = c_e[r_] - qx;
            } else {
                i64 s64 = (i64)c_s[r_] - qx64, e64 = (i64)c_e[r_] - qx64;
                s64 = s64 < -(1ll << 30) ? -(1ll << 30) : (s64 > (1ll << 30) ? (1ll << 30) : s64);
                e64 = e64 < -(1ll << 30) ? -(1ll << 30) : (e64 > (1ll << 30) ? (1ll << 30) : e64);
                sr = (int)s64; er = (int)e64;
            }
        }
        const int pe = dpp_mov<0x138, 0xf>(carry_e, er), ps = dpp_mov<0x138, 0xf>(carry_s, sr);    // wave_shr:1 (lane 0: the round before)
        if (i < n_c && (sr < pe || sr == ps)) bad = true;                   // (overlap, equal starts: not a window's business)
        const bool in = i < n_c && er > 0 && sr < wlen && er > sr;         // (an empty interval covers nothing: sets nothing)
        const int s_c = sr < 0 ? 0 : sr;
        if (in) atomicOr(&Wn.bm[s_c >> 5], 1u << (s_c & 31));
        if (in && er < wlen) atomicOr(&Wn.bm[er >> 5], 1u << (er & 31));
        const int last = (n_c - b > WAVE ? WAVE : n_c - b) - 1;
        carry_e = rdl(er, last); carry_s = rdl(sr, last);
        c_s[r_] = in ? s_c : -1;                     // (-1: sets nothing)
        c_e[r_] = (in && er < wlen) ? er : -1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (__builtin_amdgcn_ballot_w64(bad) != 0) return false;
    {   // exclusive popcount prefix over the 128 words: lane owns words 2 lane, 2 lane + 1
        const int c0 = __builtin_popcount(Wn.bm[2 * lane]), c1 = __builtin_popcount(Wn.bm[2 * lane + 1]);
        const int incl = wave_scan_inclusive<OpAdd>(c0 + c1);
        Wn.pre[2 * lane] = (u32)(incl - c0 - c1);
        Wn.pre[2 * lane + 1] = (u32)(incl - c1);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // pass 2: the values behind the breakpoints, at their ranks: ends first (0.0), then starts (an interval that starts where the
    // one in front of it ends shares its bit -- and overwrites its 0.0)
    auto rank_of = [&](const int r) -> int {
        return (int)Wn.pre[r >> 5] + __builtin_popcount(Wn.bm[r >> 5] & (0xFFFFFFFFu >> (31 - (r & 31))));
    };
#pragma unroll
    for (int r_ = 0; r_ < PAINT_TILE / WAVE; ++r_)
        if (r_ * WAVE < n_c && c_e[r_] >= 0) Wn.bv[rank_of(c_e[r_])] = 0.0f;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int r_ = 0; r_ < PAINT_TILE / WAVE; ++r_)
        if (r_ * WAVE < n_c && c_s[r_] >= 0) Wn.bv[rank_of(c_s[r_])] = c_v[r_];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    x_lo_out = x_lo; wlen_out = wlen;
    return true;
}

// PAINT: the track comes from the query's intervals (SrcPainted; A.tracks is not read), else from memory.
// The body of one chunk-wave: (row k, chunk) of n_chunks; M / Wn_ = the wave's tables in LDS; kernarg = the kernel's argument segment
// (TrackArgs, PaintSrcArgs behind it).  realign_tracks_kernel inlines it; realign_paint_kernel calls a copy of it for the chunks its
// fast path does not take.
template <bool PAINT>
__device__ __forceinline__ void realign_body(const TrackArgs &A, const PaintSrcArgs &PS_, TrackMirror &M, PaintWin &Wn_, const u64 kernarg,
                                             const i64 k, const int chunk, const int n_chunks) {
    const int lane = threadIdx.x & (WAVE - 1);
    const i64 query = A.ploidy_shift >= 0 ? (k >> A.ploidy_shift) : (i64)((u32)k / (u32)A.ploidy);
    const i64 hap = k - query * A.ploidy;
    // the row's parameters are wave-uniform: scalar loads (through the constant address space, which is what makes the
    // compiler pick s_load for a global array; as recon_lean_kernel reads its request entries)
    typedef const int __attribute__((address_space(4))) *KInt;
    typedef const i64 __attribute__((address_space(4))) *KI64;
    const i64 *oi_ptr = nullptr;
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (PAINT) {       // (the pointer itself is a kernel argument: fetched with the others, not behind round 1)
        oi_ptr = ((PaintSrcArgsK)(kernarg + sizeof(TrackArgs)))->offset_idxs;
        asm volatile("" :: "s"(oi_ptr), "s"(A.out_offsets), "s"(A.track_offsets), "s"(A.regions), "s"(A.shifts), "s"(A.geno_offset_idx));
    }
#endif
    // Round 1: everything the row's number alone addresses, requested as a whole before any of it is used (written value
    // by value, each load became a memory round trip of its own behind the branch in front of its first use).
    const i64 row_base = ((KI64)(u64)A.out_offsets)[k];
    const i64 row_end = ((KI64)(u64)A.out_offsets)[k + 1];
    const i64 t_s = ((KI64)(u64)A.track_offsets)[query << A.to_shift];
    const i64 t_e = ((KI64)(u64)A.track_offsets)[(query << A.to_shift) + 1];
    const i64 q_start = ((KInt)(u64)A.regions)[query * A.regions_stride + 1];
    const i64 shift = ((KInt)(u64)A.shifts)[k];
    const i64 o_idx = ((KI64)(u64)A.geno_offset_idx)[k];
    const bool has_keep = A.keep && A.keep_offsets;
    const i64 keep_off = has_keep ? ((KI64)(u64)A.keep_offsets)[k] : 0;
    // (to_rc is a byte array: the aligned word that holds the row's byte)
    const u64 rc_addr = (u64)A.to_rc + (u64)k;
    const int rc_word = A.to_rc ? ((KInt)(rc_addr & ~3ull))[0] : 0;
    i64 idx_raw = 0;                        // (the interval list's number)
    // (the chunk's walk state, if the caller prepared them: eight scalars of the same round)
    int ph_first = 0, ph_count = -1;
    if (A.plan_hdr) {
        const KInt w = (KInt)(u64)(A.plan_hdr + (k * (i64)n_chunks + (i64)chunk));
        ph_first = w[0]; ph_count = w[1];
    }
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (PAINT) idx_raw = ((KI64)(u64)oi_ptr)[query];
    asm volatile("" :: "s"(row_base), "s"(row_end), "s"(t_s), "s"(t_e), "s"((int)q_start), "s"((int)shift), "s"(o_idx), "s"(keep_off),
                 "s"(rc_word), "s"(idx_raw));
#endif
    // Round 2: the genotype list's bounds
    const i64 o_s = ((KI64)(u64)A.go_starts)[o_idx];
    const i64 nv64 = ((KI64)(u64)A.go_stops)[o_idx] - o_s;
    const int L = (int)(row_end - row_base);
    const int lo_clip = chunk * A.chunk_len;
    if (lo_clip >= L) return;
    const int hi_clip = (L - lo_clip > A.chunk_len) ? lo_clip + A.chunk_len : L;
    const i64 tlen = t_e - t_s;
    const float *track = PAINT ? nullptr : A.tracks + t_s;
    const int n_var = nv64 < 0 ? 0 : (nv64 > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)nv64);
    const bool rc = ((rc_word >> (8 * (int)(rc_addr & 3ull))) & 0xFF) != 0;
    float *out_row = A.out + row_base;

    int s_out = 0, s_kind = 0, s_plo = 0, s_phi = 0, s_vlen = 0;
    int nseg = 0;
    int last_kind = -1; i64 last_p = 0;
    auto push = [&](int kind, int o_start, int len, i64 pval, int vlen) {
        if (len <= 0 || o_start + len <= lo_clip || o_start >= hi_clip) return;
        if (kind == T_TRACK && last_kind == T_TRACK && pval == last_p) return;   // run continues
        if (lane == nseg) {
            s_out = o_start; s_kind = kind; s_plo = (int)(u32)(u64)pval; s_phi = (int)(u32)((u64)pval >> 32);
            s_vlen = vlen;
            M.out[lane] = o_start; M.kind[lane] = kind; M.plo[lane] = s_plo; M.phi[lane] = s_phi; M.vlen[lane] = vlen;
        }
        last_kind = kind; last_p = pval; ++nseg;
    };

    i64 track_idx = 0, shifted = 0;
    int out_idx = 0;
    int r_pos = 0, r_ilen = 0, r_keep = 1;
    int vi = 0, vb = -WAVE;
    bool walk_done = false;
    int emit_pos = lo_clip;
    if (n_var == 0) {   // src/tracks/mod.rs:240-246: out[:] = track[:length]
        push(T_TRACK, 0, L, 0, 0);
        out_idx = L;
        walk_done = true;
    }
    // The row was planned as a whole (track_plan_kernel: by the native loop with its epoch table, or once per gvl_tracks_batch
    // call): the chunk's entries are `ph_count` consecutive ones of the row's table -- one read, no walk.
    if (!walk_done && ph_count > 0 && ph_count <= SEG_CAP && !(A.dbg & (DBG_SCALAR_WALK | DBG_NO_TRACK_PLANS))) {
        if (lane < ph_count) {
            const i32x4 e = A.plan_ent[k * (i64)PLAN_MAXE + ph_first + lane];
            M.out[lane] = e.x; M.kind[lane] = (e.y == T_FILL && A.strategy == GVL_FILL_REPEAT_5P) ? (int)T_REPEAT : e.y;
            M.plo[lane] = e.z; M.phi[lane] = e.z >> 31; M.vlen[lane] = e.w;
        }
        nseg = ph_count;
        out_idx = L;
        walk_done = true;
        if (A.stamps && lane == 0) atomicAdd((unsigned long long *)&A.stamps[15], 1ull);       // chunk-waves that read their plan
    }

    // Planned walk: the same restatement as reconstruct_kernel's P3 (lane j = variant j, wave
    // scans for "first ALT wins" and the output offsets), with the track rules: SNPs only take
    // part in the shift (:312-314), every applied indel ends a track run, no lead pad.  It
    // writes the chunk's entries straight into the LDS table; anything it cannot express in
    // i32 / 64 entries leaves the table empty for the scalar walk below.
    if (!walk_done && !(A.dbg & DBG_SCALAR_WALK)) {
        bool ok = q_start > -(1ll << 30) && q_start < (1ll << 30) && shift >= 0 && shift < (1ll << 30);
        int rem = (int)(ok ? shift : 0);
        int tidx0 = 0, pm_carry = 0, x_carry = 0;
        bool ended = false, past_chunk = false;
        int tidx_end = 0, out_end = 0;
        int n_ent = 0;
        const int tb0 = 0;
        const int qs = (int)(ok ? q_start : 0);
        auto put = [&](int q, int kind, int o_start, i64 pval, int vlen) {
            if (q < SEG_CAP) {
                M.out[q] = o_start; M.kind[q] = kind; M.plo[q] = (int)(u32)(u64)pval;
                M.phi[q] = (int)(u32)((u64)pval >> 32); M.vlen[q] = vlen;
            }
        };
        // (position and length delta sit next to the CSR entry, gvl_grec: one read, not three; a trip's records are
        // requested a trip ahead)
        int nxt_pos = 0, nxt_d = 0;
        if (A.grec && tb0 + lane < n_var) {
            const i32x4 rec = *reinterpret_cast<const i32x4 *>(A.grec + (o_s + tb0 + lane));
            nxt_pos = rec.x; nxt_d = rec.y;
        }
        for (int tb = tb0; tb < n_var && ok && !ended && !past_chunk; tb += WAVE) {
            int pos = 0, d = 0;
            bool valid = tb + lane < n_var;
            const int rec_pos = nxt_pos, rec_d = nxt_d;
            if (A.grec && tb + WAVE + lane < n_var) {
                const i32x4 rec = *reinterpret_cast<const i32x4 *>(A.grec + (o_s + tb + WAVE + lane));
                nxt_pos = rec.x; nxt_d = rec.y;
            }
            if (valid) {
                if (A.grec) {
                    pos = rec_pos; d = rec_d;
                } else {
                    int v = A.geno_v_idxs[o_s + tb + lane];
                    v = v < 0 ? 0 : ((i64)v >= A.n_variants ? (int)(A.n_variants - 1) : v);
                    pos = A.v_starts[v]; d = A.ilens[v];
                }
                if (has_keep) valid = A.keep[keep_off + tb + lane] != 0;
            }
            const bool weird = valid && (pos <= -(1 << 30) || pos >= (1 << 30) || d <= -(1 << 30) || d >= (1 << 30));
            ok = ok && __builtin_amdgcn_ballot_w64(weird) == 0;
            const int vrp = pos - qs;                                   // :264
            const int E = vrp - (d < 0 ? d : 0) + 1;                    // :267
            int v_len = (d > 0 ? d : 0) + 1;                            // :282
            const u64 m_span = __builtin_amdgcn_ballot_w64(valid && d < 0 && vrp < 0 && E >= 0);   // :271-274
            if (m_span) { tidx0 = rdl(E, 63 - __builtin_clzll(m_span)); pm_carry = tidx0; tidx_end = tidx0; }
            bool cand = valid && vrp >= 0;
            if (rem > 0) {                                              // :285-308
                const int base = tidx0;
                const u64 m_t = __builtin_amdgcn_ballot_w64(cand && vrp >= base && (vrp - base) + v_len >= rem);
                if (m_t == 0) {
                    cand = false;
                } else {
                    const int f = __builtin_ctzll(m_t);
                    const int dist = rdl(vrp, f) - base;
                    if (dist >= rem) {
                        tidx0 = base + rem;
                        cand = cand && lane >= f;
                    } else {
                        const int skip = rem - dist;
                        if (skip == rdl(v_len, f)) {
                            tidx0 = rdl(E, f);
                            cand = cand && lane > f;
                        } else {
                            tidx0 = rdl(vrp, f);
                            cand = cand && lane >= f;
                            if (lane == f) v_len -= skip;
                        }
                    }
                    rem = 0;
                    pm_carry = tidx0; tidx_end = tidx0;
                }
            }
            cand = cand && d != 0;                                      // :312-314
            bool inB = cand;
            int PM = 0, pm_incl = 0;
            {
                u64 mB = __builtin_amdgcn_ballot_w64(inB);
                bool stable = false;
#pragma unroll 1
                for (int it = 0; it < 4 && !stable; ++it) {
                    PM = wave_scan_exclusive<OpMaxU>(inB ? E : 0, pm_incl);
                    PM = PM > pm_carry ? PM : pm_carry;
                    inB = cand && vrp >= PM;                            // :277-279
                    const u64 m2 = __builtin_amdgcn_ballot_w64(inB);
                    stable = m2 == mB;
                    mB = m2;
                }
                ok = ok && stable;
            }
            const int n_i = inB ? vrp - PM : 0;                         // :317
            const int S_i = inB ? OpSat::f(n_i, v_len) : 0;
            int x_incl;
            const int X = OpSat::f(x_carry, wave_scan_exclusive<OpSat>(S_i, x_incl));   // out_idx before this variant
            const int fill_out = OpSat::f(X, n_i);
            const bool applied = inB && fill_out < L;                   // :319-321 break
            const int w_i = applied ? ((v_len < L - fill_out) ? v_len : L - fill_out) : 0;   // :329
            const u64 m_inB = __builtin_amdgcn_ballot_w64(inB);
            const u64 m_app = __builtin_amdgcn_ballot_w64(applied);
            if (m_inB != m_app) ended = true;
            if (m_app) {
                const int last = 63 - __builtin_clzll(m_app);
                tidx_end = rdl(E, last);
                out_end = rdl(fill_out, last) + rdl(w_i, last);
                if (rdl(fill_out, last) >= hi_clip) past_chunk = true;
            }
            const bool e_trk = applied && n_i > 0 && fill_out > lo_clip && X < hi_clip;
            const bool e_fil = applied && w_i > 0 && fill_out + w_i > lo_clip && fill_out < hi_clip;
            const int slot0 = n_ent + wave_scan_exclusive<OpAdd>((e_trk ? 1 : 0) + (e_fil ? 1 : 0));
            const int add_ent = __builtin_popcountll(__builtin_amdgcn_ballot_w64(e_trk)) +
                                __builtin_popcountll(__builtin_amdgcn_ballot_w64(e_fil));
            if (n_ent + add_ent + 2 > SEG_CAP) ok = false;
            if (ok) {
                int q = slot0;
                if (e_trk) { put(q, T_TRACK, X, (i64)PM - X, 0); ++q; }
                if (e_fil) put(q, (d > 0 && A.strategy != GVL_FILL_REPEAT_5P) ? T_FILL : T_REPEAT, fill_out, (i64)vrp, v_len);
            }
            if (tb + WAVE < n_var) {
                const int mx = rdl(pm_incl, 63);
                pm_carry = mx > pm_carry ? mx : pm_carry;
                x_carry = OpSat::f(x_carry, rdl(x_incl, 63));
            }
            n_ent += add_ent;
        }
        if (ok) {
            if (!(past_chunk && !ended)) {                              // :365-392 tail
                i64 t_idx = tidx_end;
                if (rem > 0) t_idx = imin((i64)tidx0 + rem, tlen);
                const int u = L - out_end;
                if (u > 0 && lane == 0) {
                    const i64 avail = tlen - t_idx;
                    const int w = (int)imin((i64)u, avail);
                    int end = out_end;
                    int q = n_ent;
                    if (w > 0) {
                        end += w;
                        if (end > lo_clip && out_end < hi_clip) { put(q, T_TRACK, out_end, t_idx - out_end, 0); ++q; }
                    }
                    if (end < L && L > lo_clip && end < hi_clip) { put(q, T_ZERO, end, 0, 0); ++q; }
                    n_ent = q;
                }
                n_ent = rfl(n_ent);
            }
            nseg = n_ent;
            out_idx = L;
            walk_done = true;
        }
    }

    typename std::conditional<PAINT, SrcPainted, SrcGlobal>::type S;
    bool have_win = false;
    if constexpr (PAINT) {
#if defined(__HIP_DEVICE_COMPILE__)
        const PaintSrcArgsK PSk = (PaintSrcArgsK)(kernarg + sizeof(TrackArgs));
        const i64 dv = PSk->list_div;
        const i64 idx = dv == 1 ? idx_raw : rfl64(idx_raw / dv);
#else
        const i64 idx = 0;
#endif
        S.W = &Wn_; S.x_lo = 0; S.wlen = 0; S.win_ok = false;
        S.tlen = tlen; S.qs = q_start; S.idx = idx;
        S.ps_kernarg = kernarg + sizeof(TrackArgs);
        S.stamps = A.stamps;
    } else {
        S.track = track; S.tlen = tlen;
    }
    // the window of a painted source: from where the chunk's first value comes from on (see SrcPainted)
    auto build_window = [&](const i64 x_first) {
        if constexpr (PAINT) {
#if defined(__HIP_DEVICE_COMPILE__)
            const PaintSrcArgsK PS = (PaintSrcArgsK)(kernarg + sizeof(TrackArgs));
#else
            const PaintSrcArgs *const PS = &PS_;
#endif
            i64 x_lo = 0; int wlen = 0;
            if (paint_build_window(Wn_, PS, S.idx, q_start, tlen, x_first, lane, x_lo, wlen)) { S.x_lo = x_lo; S.wlen = wlen; S.win_ok = !(A.dbg & DBG_NO_REALIGN_WINDOW); }
        }
    };

    if (A.stamps && lane == 0) {
        atomicAdd((unsigned long long *)&A.stamps[8], 1ull);                       // chunk-waves
        if (!walk_done) atomicAdd((unsigned long long *)&A.stamps[9], 1ull);       // ... that replay the walk on the scalar unit
    }
    for (;;) {
        while (!walk_done && nseg <= SEG_FLUSH) {
            bool stop = (vi >= n_var) || (out_idx >= hi_clip);
            if (!stop) {
                if (vi - vb >= WAVE) {
                    vb = vi;
                    const int j = vb + lane;
                    if (j < n_var) {
                        if (A.grec) {
                            const i32x4 rec = *reinterpret_cast<const i32x4 *>(A.grec + (o_s + j));
                            r_pos = rec.x; r_ilen = rec.y;
                        } else {
                            int v = A.geno_v_idxs[o_s + j];
                            v = v < 0 ? 0 : ((i64)v >= A.n_variants ? (int)(A.n_variants - 1) : v);
                            r_pos = A.v_starts[v]; r_ilen = A.ilens[v];
                        }
                        r_keep = has_keep ? (int)A.keep[keep_off + j] : 1;
                    }
                }
                const int i = vi - vb;
                ++vi;
                if (has_keep && rdl(r_keep, i) == 0) continue;
                const i64 vrp = (i64)rdl(r_pos, i) - q_start;           // mod.rs:264
                const i64 d = rdl(r_ilen, i);
                const i64 vre = vrp - (d < 0 ? d : 0) + 1;               // :267
                if (d < 0 && vrp < 0 && vre >= 0) { track_idx = vre; continue; }   // :271-274
                if (vrp < track_idx) continue;                          // :277-279
                i64 v_len = (d > 0 ? d : 0) + 1;                         // :282
                if (shifted < shift) {                                   // :285-308
                    const i64 dist = vrp - track_idx;
                    if (shifted + dist + v_len < shift) continue;
                    if (shifted + dist >= shift) {
                        track_idx += shift - shifted;
                        shifted = shift;
                    } else {
                        const i64 a0 = shift - shifted - dist;
                        shifted = shift;
                        if (a0 == v_len) { track_idx = vre; continue; }
                        track_idx = vrp;
                        v_len -= a0;
                    }
                }
                if (d == 0) continue;                                    // :312-314 SNPs do not move tracks
                const i64 n64 = vrp - track_idx;
                if (n64 >= (i64)(L - out_idx)) {                          // :319-321
                    stop = true;
                } else {
                    const int n = (int)n64;
                    push(T_TRACK, out_idx, n, track_idx - out_idx, 0);
                    out_idx += n;
                    const int w = (int)imin(v_len, (i64)(L - out_idx));  // :329
                    const int vl = (int)imin(v_len, 0x7FFFFFFFll);
                    if (d > 0 && A.strategy != GVL_FILL_REPEAT_5P) push(T_FILL, out_idx, w, vrp, vl);   // :333-346
                    else push(T_REPEAT, out_idx, w, vrp, vl);            // :347-354
                    out_idx += w;
                    track_idx = vre;
                    if (out_idx >= L) stop = true;
                }
            }
            if (stop) {
                if (shifted < shift) track_idx = imin(track_idx + (shift - shifted), tlen);   // :365-369
                const int u = L - out_idx;
                if (u > 0) {
                    const int w = (int)imin((i64)u, tlen - track_idx);
                    int end = out_idx;
                    if (w > 0) { push(T_TRACK, out_idx, w, track_idx - out_idx, 0); end += w; }
                    if (end < L) push(T_ZERO, end, L - end, 0, 0);
                }
                out_idx = out_idx > L ? out_idx : L;
                walk_done = true;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        const int cov = out_idx < lo_clip ? lo_clip : (out_idx > hi_clip ? hi_clip : out_idx);
        const int limit = walk_done ? hi_clip : (cov & ~3);
        if (A.dbg & GVL_ABL(DBG_ABL_TRACK_WALK)) return;              // (timing ablation: head + walk only)
        if (PAINT && !have_win && nseg > 0) {
            // the first entry that reaches into the chunk says where its first value comes from
            // (entry 0: the table only holds entries that reach into what is still to be emitted)
            have_win = true;
            const i64 pv = (i64)(((u64)(u32)rfl(M.phi[0]) << 32) | (u32)rfl(M.plo[0]));
            build_window(rfl(M.kind[0]) == T_TRACK ? pv + emit_pos : pv);
        }
        // The round's entries, lane t = entry t (they are few: a chunk with one indel is run | fill | run); what a trip needs of
        // them is wave-uniform -- the entry its first position lies in (a ballot over the starts), that entry's kind, delta and
        // end (readlanes) -- so a trip inside ONE track run, which is all of them in a chunk without an indel and most in any
        // other, needs no per-lane lookup however long the table is.  (Until round 4 only tables of <= 4 entries were
        // dispatched this way, with their starts held in scalar registers: a chunk with two indels took the per-lane path on all
        // of its trips -- 6.5 % of BASELINE config 4's chunk-waves, two thirds of that path's trips.)
        const bool ev = lane < nseg;
        // (kind + 256: the entry's delta does not fit 32 bits -- its high word and a fill's length stay in LDS, read where needed)
        const int e_out = ev ? M.out[lane] : 0x7FFFFFFF, e_plo = ev ? M.plo[lane] : 0;
        const int e_kind = ev ? (M.kind[lane] | (M.phi[lane] == (e_plo >> 31) ? 0 : 256)) : T_ZERO;
        const bool tl32 = tlen < 0x7FFFFF00ll;
        if (A.dbg & GVL_ABL(DBG_ABL_TRACK_WINDOW)) return;             // (timing ablation: ... + the window)
        if (A.stamps && lane == 0) {
            if (PAINT && !S_win_ok(S)) atomicAdd((unsigned long long *)&A.stamps[10], 1ull);     // ... without a window
            if (nseg > 4) atomicAdd((unsigned long long *)&A.stamps[11], 1ull);                   // ... with more than 4 entries
            atomicAdd((unsigned long long *)&A.stamps[12], (unsigned long long)nseg);
        }
        int p0 = emit_pos;
        while (p0 < limit) {
            // the entry p0 lies in: the last one that starts at or in front of it
            int li = __builtin_popcountll(__builtin_amdgcn_ballot_w64(ev && e_out <= p0)) - 1;
            li = li < 0 ? 0 : li;
            {
                const int kd = rdl(e_kind, li), plo = rdl(e_plo, li);
                int nx = li + 1 < nseg ? rdl(e_out, li + 1) : cov;
                nx = nx < cov ? nx : cov;
                const int run_end = nx < limit ? nx : limit;
                if (nseg > 0 && kd == T_TRACK && tl32 && run_end - p0 >= TRIP) {
                    const i64 xs0 = (i64)plo + p0;
                    const int n2 = (run_end - p0) / (2 * TRIP);
                    // the run's double trips in a tight loop -- position and output pointer advance by a constant, nothing is
                    // selected per trip, eight values per lane (half the lookups per value)
                    // (a painted source: only runs that lie inside the window -- all of them but a chunk's last when a deletion made it
                    // longer than the window; those take the trip-by-trip form below -- so that the loop is winN's straight-line code)
                    if (n2 > 0 && xs0 >= 0 && xs0 + (i64)n2 * (2 * TRIP) <= tlen && (!PAINT || S.covers(xs0, (i64)n2 * (2 * TRIP)))) {
                        // Looked up as they are stored: every lane the four values of its group in each of the double trip's two trips
                        // -- two 16-byte stores per lane, ONE contiguous KB per store instruction (stored eight consecutive values per
                        // lane, every store instruction wrote 64 half-lines: measured in round 4, that pattern cost the kernel 10 of its
                        // 49 us; round 4 looked eight up and transposed them through LDS -- the second lookup is cheaper than the
                        // transposition since a lookup is a popcount and a read, and the kernel's LDS drops from 25.7 to 17.5 KB a
                        // workgroup: 8 waves per SIMD fit)
                        int x = (int)xs0 + GROUP * lane - (PAINT ? (int)S.x_lo : 0);       // (PAINT: a window position)
                        float *o = rc ? out_row + (L - GROUP - (p0 + GROUP * lane)) : out_row + (p0 + GROUP * lane);
                        const int ostep = rc ? -2 * TRIP : 2 * TRIP;
#pragma unroll 1
                        for (int i = 0; i < n2; ++i) {
                            float q1[GROUP], q2[GROUP];
                            if constexpr (PAINT) { S.template winN<GROUP>(x, q1); S.template winN<GROUP>(x + TRIP, q2); }
                            else { S.at4i(x, q1); S.at4i(x + TRIP, q2); }
                            if (!rc) {
                                store_f32x4(o, q1[0], q1[1], q1[2], q1[3]);
                                store_f32x4(o + TRIP, q2[0], q2[1], q2[2], q2[3]);
                            } else {
                                store_f32x4(o, q1[3], q1[2], q1[1], q1[0]);
                                store_f32x4(o - TRIP, q2[3], q2[2], q2[1], q2[0]);
                            }
                            x += 2 * TRIP; o += ostep;
                        }
                        p0 += n2 * (2 * TRIP);
                        continue;
                    }
                    if (xs0 >= 0 && xs0 + TRIP <= tlen) {       // one trip of the run
                        float v4[GROUP];
                        const int p = p0 + GROUP * lane;
                        S.at4i((int)xs0 + GROUP * lane, v4);
                        if (!rc) store_f32x4(out_row + p, v4[0], v4[1], v4[2], v4[3]);
                        else store_f32x4(out_row + (L - GROUP - p), v4[3], v4[2], v4[1], v4[0]);
                        p0 += TRIP;
                        continue;
                    }
                }
            }
            // A trip that crosses entries (or reaches the row's end, or a track's): entry by entry, each wave-uniform -- its
            // kind, delta and range are scalars, a lane takes from it the positions of its group that lie inside.
            if (A.stamps && lane == 0) atomicAdd((unsigned long long *)&A.stamps[13], 1ull);    // trips on this path
            const int p = p0 + GROUP * lane;
            float v4[GROUP];
#pragma unroll
            for (int g = 0; g < GROUP; ++g) v4[g] = 0.0f;
            const int trip_end = (limit - p0 > TRIP) ? p0 + TRIP : limit;
            if (nseg > 0) {
#pragma unroll 1
                for (;;) {
                    const int st_e = rdl(e_out, li), kd = rdl(e_kind, li) & 255;
                    const i64 pv = (i64)(((u64)(u32)rfl(M.phi[li]) << 32) | (u32)rdl(e_plo, li));
                    int nx = li + 1 < nseg ? rdl(e_out, li + 1) : cov;
                    nx = nx < trip_end ? nx : trip_end;
                    const bool mine = p + GROUP > st_e && p < nx;              // some position of the lane's group is this entry's
                    float t4[GROUP];
#pragma unroll
                    for (int g = 0; g < GROUP; ++g) t4[g] = 0.0f;
                    if (kd == T_TRACK) {
                        if (mine) {
                            const i64 x = pv + p;
                            if (x >= 0 && x + GROUP <= tlen) {
                                S.at4(x, t4);
                            } else {
#pragma unroll
                                for (int g = 0; g < GROUP; ++g) t4[g] = S.at(x + g);
                            }
                        }
                    } else if (kd == T_REPEAT) {
                        const float v = S.at(pv);                               // (one position for the whole entry)
#pragma unroll
                        for (int g = 0; g < GROUP; ++g) t4[g] = v;
                    } else if (kd == T_FILL) {
                        const i64 vl = (i64)rfl(M.vlen[li]);
#pragma unroll
                        for (int g = 0; g < GROUP; ++g) {
                            const int pp = p + g;
                            if (pp >= st_e && pp < nx) t4[g] = fill_value(A, S, pv, vl, (i64)(pp - st_e), (i64)pp, (u64)query, (u64)hap);
                        }
                    }
#pragma unroll
                    for (int g = 0; g < GROUP; ++g)
                        if (p + g >= st_e && p + g < nx) v4[g] = t4[g];
                    if (nx >= trip_end || li + 1 >= nseg) break;
                    ++li;
                }
            }
            if (p + GROUP <= limit) {
                if (!rc) store_f32x4(out_row + p, v4[0], v4[1], v4[2], v4[3]);
                else store_f32x4(out_row + (L - GROUP - p), v4[3], v4[2], v4[1], v4[0]);
            } else {
#pragma unroll
                for (int i = 0; i < GROUP; ++i)
                    if (p + i < limit) out_row[rc ? (L - 1 - (p + i)) : (p + i)] = v4[i];
            }
            p0 += TRIP;
        }
        emit_pos = limit;
        if (walk_done || emit_pos >= hi_clip) break;
        {   // compact: keep the segment that holds emit_pos and everything after it
            int cnt = 0;
            for (int s2 = 0; s2 < nseg; ++s2) cnt += (rdl(s_out, s2) <= emit_pos) ? 1 : 0;
            const int s0 = cnt > 0 ? cnt - 1 : 0;
            if (s0 > 0) {
                const int srcl = lane + s0 < SEG_CAP ? lane + s0 : SEG_CAP - 1;
                s_out = bperm(srcl, s_out); s_kind = bperm(srcl, s_kind); s_plo = bperm(srcl, s_plo);
                s_phi = bperm(srcl, s_phi); s_vlen = bperm(srcl, s_vlen);
                nseg -= s0;
            }
            M.out[lane] = s_out; M.kind[lane] = s_kind; M.plo[lane] = s_plo; M.phi[lane] = s_phi; M.vlen[lane] = s_vlen;
        }
    }
}

// (8 waves per SIMD: 63 VGPRs + 17.5 KB of LDS a workgroup; at the 6 the compiler picks by itself -- 75 VGPRs -- the kernel is 0.5 us slower)
template <bool PAINT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void realign_tracks_kernel(const TrackArgs A, const PaintSrcArgs PS_) {
    __shared__ TrackMirror mirror[4];
    __shared__ PaintWin wins[PAINT ? 4 : 1];
    const int wave = rfl((int)(threadIdx.x >> 6));
    const i64 k = (i64)blockIdx.x * 4 + wave;
    if (k >= A.n_rows) return;
    realign_body<PAINT>(A, PS_, mirror[wave], wins[PAINT ? wave : 0], (u64)__builtin_amdgcn_kernarg_segment_ptr(), k, (int)blockIdx.y, (int)gridDim.y);
}

// ---- ragged rows: the 1-D launches over a batch's chunk list --------------------------------------------------------------------------
// A batch of mixed row lengths launched over rows x ceil(max_row_len / chunk_len) is mostly chunk-waves past their row's end.
// track_chunk_list_kernel lists the (row, chunk) pairs that hold values, in row order; the list kernels below take them in a
// grid-stride loop, wave by wave, with at most CHUNK_LIST_WGS workgroups (one full residency of the chip at 8 waves per SIMD).
// Their arguments start with the 2-D kernels' (TrackArgs, PaintSrcArgs): realign_chunk_general finds them at the same offsets.
constexpr int CHUNK_LIST_WGS = 2048;
__global__ __launch_bounds__(1024) void track_chunk_list_kernel(const i64 *out_offsets, i64 n_rows, int chunk_len, int chunks, i64 max_row_len,
                                                                i64 cap, int2 *list, int *count, int *async_err) {
    __shared__ int wsum[16];
    __shared__ int carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (i64 base = 0; base < n_rows; base += 1024) {
        const i64 k = base + tid;
        int nc = 0;
        if (k < n_rows) {
            const i64 o0 = out_offsets[k], o1 = out_offsets[k + 1], len = o1 - o0;
            // (a row outside the output, or longer than the bound the launch was sized for: cut or left out, and reported)
            if (o0 < 0 || len < 0 || o1 > cap) {
                atomicOr(async_err, 1);
            } else {
                if (len > max_row_len) atomicOr(async_err, 1);
                const i64 c = (len + chunk_len - 1) / chunk_len;
                nc = (int)(c < chunks ? c : chunks);
            }
        }
        int s = nc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(s, o, 64);
            if (lane >= o) s += y;
        }
        if (lane == 63) wsum[wv] = s;
        __syncthreads();
        int pre = carry_s;
        for (int w = 0; w < wv; ++w) pre += wsum[w];
        for (int c = 0; c < nc; ++c) list[pre + s - nc + c] = make_int2((int)k, c);
        __syncthreads();
        if (tid == 1023) carry_s = pre + s;
        __syncthreads();
    }
    if (tid == 0) *count = carry_s;
}

template <bool PAINT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void realign_tracks_list_kernel(const TrackArgs A, const PaintSrcArgs PS_,
                                                                                                              const int2 *list, const int *count, const int n_chunks) {
    __shared__ TrackMirror mirror[4];
    __shared__ PaintWin wins[PAINT ? 4 : 1];
    const int wave = rfl((int)(threadIdx.x >> 6));
    const i64 n = rfl(*count);
    for (i64 e = (i64)blockIdx.x * 4 + wave; e < n; e += (i64)gridDim.x * 4) {
        const int2 kc = list[e];
        realign_body<PAINT>(A, PS_, mirror[wave], wins[PAINT ? wave : 0], (u64)__builtin_amdgcn_kernarg_segment_ptr(), (i64)rfl(kc.x), rfl(kc.y), n_chunks);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // (the wave's LDS tables are the next entry's)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ---- BASELINE config 4's track kernel: tracks straight from the intervals, rows planned ahead --------------------------------------
// realign_tracks_kernel<PAINT> can write any chunk of any row -- it carries the planned walk, the scalar walk with its flush and
// compaction, every fill strategy, 64-bit deltas, lookups in the interval list itself -- and pays for it on every chunk: its scalar
// state does not fit 8 waves' worth of SGPRs (174 spilled: a third of the kernel's 3 700 VALU instructions are v_readlane / v_writelane)
// and its head reads a dozen arrays the planned path never uses.  realign_paint_kernel is the path almost every chunk of a planned
// epoch takes, and nothing else: the chunk's entries come from the row's plan (track_plan_kernel), every value from the wave's window
// (a popcount and one LDS read, PaintWin), runs / repeats / zeros only.  A chunk that needs anything more -- no plan, a fill strategy
// that is evaluated per position, a source position outside the window or the track, a window that cannot be built -- calls the
// general body for itself (a real call: the fast path's registers are not the general body's).  Results are the general kernel's.
typedef const TrackArgs __attribute__((address_space(4))) *TrackArgsK;
typedef TrackMirror __attribute__((address_space(3))) *TrackMirrorLds;
typedef PaintWin __attribute__((address_space(3))) *PaintWinLds;
__device__ __noinline__ void realign_chunk_general(const u64 kernarg, const TrackMirrorLds m_lds, const PaintWinLds w_lds, const i64 k, const int chunk,
                                                   const int n_chunks) {
#if defined(__HIP_DEVICE_COMPILE__)
    const TrackArgs A = *(TrackArgsK)(u64)rfl64((i64)kernarg);
    const PaintSrcArgs PS = *(PaintSrcArgsK)(u64)(rfl64((i64)kernarg) + (i64)sizeof(TrackArgs));
    realign_body<true>(A, PS, *(TrackMirror *)m_lds, *(PaintWin *)w_lds, (u64)rfl64((i64)kernarg), rfl64(k), rfl(chunk), rfl(n_chunks));
#endif
}

// (diagnostic builds with gvl_diag_set_stamps and DBG_PAINT_TIMELINE: a timeline -- 8 u64 per (row, chunk) behind the 64 counters, s_memrealtime
// (100 MHz) at the wave's start [0], window built [3], stores issued [5]: tools/stamps_paint.py.  Three stamps only: each is a scalar
// memory operation, and a wait behind it serialises the head's rounds of scalar loads; the counters' same-address atomics are off then)
#ifdef GVL_DIAG
#define PAINT_STAMP(i) do { if (tl_on && lane == 0) A.stamps[64 + (k * (i64)n_chunks + chunk) * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define PAINT_STAMP(i) do { } while (0)
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void realign_paint_kernel(const TrackArgs A, const PaintSrcArgs PS_) {
    __shared__ TrackMirror mirror[4];          // (the general body's table: only chunks that leave the fast path touch it)
    __shared__ PaintWin wins[4];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const i64 k = (i64)blockIdx.x * 4 + wave;
    if (k >= A.n_rows) return;
    const int chunk = blockIdx.y;
    const int n_chunks = gridDim.y;
#include "gvl_paint_chunk.inc"
}
// (the same body over a chunk list, in a lambda: its returns end the entry, not the wave.  The body is included, not called, so that
// the 2-D kernel above compiles to the code it had before the list form existed)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void realign_paint_list_kernel(const TrackArgs A, const PaintSrcArgs PS_,
                                                                                                             const int2 *list, const int *count, const int n_chunks) {
    __shared__ TrackMirror mirror[4];
    __shared__ PaintWin wins[4];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const i64 n = rfl(*count);
    for (i64 e = (i64)blockIdx.x * 4 + wave; e < n; e += (i64)gridDim.x * 4) {
        const int2 kc = list[e];
        const i64 k = (i64)rfl(kc.x);
        const int chunk = rfl(kc.y);
        [&]() {
#include "gvl_paint_chunk.inc"
        }();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // (the wave's LDS tables are the next entry's)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}
#undef PAINT_STAMP

// ---- row plans: realign_tracks_kernel's planned walk over a WHOLE row, once: every entry of the row into a table in memory
// (at most PLAN_MAXE; 32-bit deltas), and per chunk of the row which of them reach into it.  The kernel's chunk-waves then read
// their entries instead of walking: BASELINE config 4 has 176 variants per row = 3 trips of 64, of which a chunk-wave ran 2.2 on
// average (wave scans, ballots, the records' loads: a quarter of the kernel's instructions) to find the 1.8 entries it
// needs.  One wave per row; a row the planned walk cannot express, with more entries than the table holds or with a delta
// beyond 32 bits is marked unplanned (count -1): its chunk-waves walk as before.
// (BLOCKED: ragged rows of the loader's epoch table, row offsets per batch -- see below; the other form is the fixed-length / per-call one)
template <bool BLOCKED>
__global__ __launch_bounds__(256) void track_plan_kernel(const TrackArgs A, int2 *hdr, i32x4 *ent_all, const int chunks, const i64 fixed_len,
                                                          const i64 tl_bs) {
    __shared__ int outs[4][PLAN_MAXE];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const i64 k = (i64)blockIdx.x * 4 + wave;
    if (k >= A.n_rows) return;
    const i64 query = A.ploidy_shift >= 0 ? (k >> A.ploidy_shift) : (i64)((u32)k / (u32)A.ploidy);
    // (fixed_len >= 0: every row has that length -- the loader's epoch table has no row offsets; BLOCKED: every batch of tl_bs
    // queries has its own tl_bs * ploidy + 1 row offsets)
    const i64 ko = BLOCKED ? k + k / (tl_bs * A.ploidy) : k;
    const i64 row_base = fixed_len >= 0 ? 0 : A.out_offsets[ko], row_end = fixed_len >= 0 ? fixed_len : A.out_offsets[ko + 1];
    const i64 q_start = A.regions[query * A.regions_stride + 1];
    const i64 shift = A.shifts[k];
    const i64 o_idx = A.geno_offset_idx[k];
    const bool has_keep = A.keep && A.keep_offsets;
    const i64 keep_off = has_keep ? A.keep_offsets[k] : 0;
    const i64 o_s = A.go_starts[o_idx];
    const i64 nv64 = A.go_stops[o_idx] - o_s;
    const i64 L64 = row_end - row_base;
    const int L = (int)L64;
    const int n_var = nv64 < 0 ? 0 : (nv64 > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)nv64);
    // (tl_bs > 0: the loader's epoch table -- every batch of tl_bs queries has its own tl_bs + 1 offsets)
    const i64 tq = tl_bs > 0 ? query + query / tl_bs : (query << A.to_shift);
    const i64 tlen = A.track_offsets[tq + 1] - A.track_offsets[tq];
    i32x4 *const ent = ent_all + k * (i64)PLAN_MAXE;
    bool ok = q_start > -(1ll << 30) && q_start < (1ll << 30) && shift >= 0 && shift < (1ll << 30) && !(A.dbg & DBG_SCALAR_WALK) && n_var > 0 &&
              L64 > 0 && L64 < 0x7FFFFF00ll;
    int rem = (int)(ok ? shift : 0);
    int tidx0 = 0, pm_carry = 0, x_carry = 0;
    bool ended = false;
    int tidx_end = 0, out_end = 0;
    int n_ent = 0;
    const int qs = (int)(ok ? q_start : 0);
    auto put = [&](int q, int kind, int o_start, i64 pval, int vlen) {
        if (q < PLAN_MAXE) {
            const i32x4 e = {o_start, kind, (int)pval, vlen};
            ent[q] = e;
            outs[wave][q] = o_start;
        }
    };
    for (int tb = 0; tb < n_var && ok && !ended; tb += WAVE) {
        int pos = 0, d = 0;
        bool valid = tb + lane < n_var;
        if (valid) {
            if (A.grec) {
                const i32x4 rec = *reinterpret_cast<const i32x4 *>(A.grec + (o_s + tb + lane));
                pos = rec.x; d = rec.y;
            } else {
                int v = A.geno_v_idxs[o_s + tb + lane];
                v = v < 0 ? 0 : ((i64)v >= A.n_variants ? (int)(A.n_variants - 1) : v);
                pos = A.v_starts[v]; d = A.ilens[v];
            }
            if (has_keep) valid = A.keep[keep_off + tb + lane] != 0;
        }
        const bool weird = valid && (pos <= -(1 << 30) || pos >= (1 << 30) || d <= -(1 << 30) || d >= (1 << 30));
        ok = ok && __builtin_amdgcn_ballot_w64(weird) == 0;
        const int vrp = pos - qs;
        const int E = vrp - (d < 0 ? d : 0) + 1;
        int v_len = (d > 0 ? d : 0) + 1;
        const u64 m_span = __builtin_amdgcn_ballot_w64(valid && d < 0 && vrp < 0 && E >= 0);
        if (m_span) { tidx0 = rdl(E, 63 - __builtin_clzll(m_span)); pm_carry = tidx0; tidx_end = tidx0; }
        bool cand = valid && vrp >= 0;
        if (rem > 0) {
            const int base = tidx0;
            const u64 m_t = __builtin_amdgcn_ballot_w64(cand && vrp >= base && (vrp - base) + v_len >= rem);
            if (m_t == 0) {
                cand = false;
            } else {
                const int f = __builtin_ctzll(m_t);
                const int dist = rdl(vrp, f) - base;
                if (dist >= rem) {
                    tidx0 = base + rem;
                    cand = cand && lane >= f;
                } else {
                    const int skip = rem - dist;
                    if (skip == rdl(v_len, f)) {
                        tidx0 = rdl(E, f);
                        cand = cand && lane > f;
                    } else {
                        tidx0 = rdl(vrp, f);
                        cand = cand && lane >= f;
                        if (lane == f) v_len -= skip;
                    }
                }
                rem = 0;
                pm_carry = tidx0; tidx_end = tidx0;
            }
        }
        cand = cand && d != 0;
        bool inB = cand;
        int PM = 0, pm_incl = 0;
        {
            u64 mB = __builtin_amdgcn_ballot_w64(inB);
            bool stable = false;
#pragma unroll 1
            for (int it = 0; it < 4 && !stable; ++it) {
                PM = wave_scan_exclusive<OpMaxU>(inB ? E : 0, pm_incl);
                PM = PM > pm_carry ? PM : pm_carry;
                inB = cand && vrp >= PM;
                const u64 m2 = __builtin_amdgcn_ballot_w64(inB);
                stable = m2 == mB;
                mB = m2;
            }
            ok = ok && stable;
        }
        const int n_i = inB ? vrp - PM : 0;
        const int S_i = inB ? OpSat::f(n_i, v_len) : 0;
        int x_incl;
        const int X = OpSat::f(x_carry, wave_scan_exclusive<OpSat>(S_i, x_incl));
        const int fill_out = OpSat::f(X, n_i);
        const bool applied = inB && fill_out < L;
        const int w_i = applied ? ((v_len < L - fill_out) ? v_len : L - fill_out) : 0;
        const u64 m_inB = __builtin_amdgcn_ballot_w64(inB);
        const u64 m_app = __builtin_amdgcn_ballot_w64(applied);
        if (m_inB != m_app) ended = true;
        if (m_app) {
            const int last = 63 - __builtin_clzll(m_app);
            tidx_end = rdl(E, last);
            out_end = rdl(fill_out, last) + rdl(w_i, last);
        }
        // (the whole row is "the chunk": every run in front of an applied variant, every fill)
        const bool e_trk = applied && n_i > 0 && fill_out > 0;
        const bool e_fil = applied && w_i > 0;
        const int slot0 = n_ent + wave_scan_exclusive<OpAdd>((e_trk ? 1 : 0) + (e_fil ? 1 : 0));
        const int add_ent = __builtin_popcountll(__builtin_amdgcn_ballot_w64(e_trk)) +
                            __builtin_popcountll(__builtin_amdgcn_ballot_w64(e_fil));
        if (n_ent + add_ent + 2 > PLAN_MAXE) ok = false;
        if (ok) {
            int q = slot0;
            if (e_trk) { put(q, T_TRACK, X, (i64)PM - X, 0); ++q; }
            // (an insertion is T_FILL here whatever the fill: the plan serves every track of the batch, and a track may have
            // its own strategy -- the reader turns it into T_REPEAT for Repeat5p)
            if (e_fil) put(q, d > 0 ? T_FILL : T_REPEAT, fill_out, (i64)vrp, v_len);
        }
        if (tb + WAVE < n_var) {
            const int mx = rdl(pm_incl, 63);
            pm_carry = mx > pm_carry ? mx : pm_carry;
            x_carry = OpSat::f(x_carry, rdl(x_incl, 63));
        }
        n_ent += add_ent;
    }
    if (ok) {      // src/tracks/mod.rs:365-392: the tail
        i64 t_idx = tidx_end;
        if (rem > 0) t_idx = imin((i64)tidx0 + rem, tlen);
        const int u = L - out_end;
        if (u > 0 && lane == 0) {
            const i64 avail = tlen - t_idx;
            const int w = (int)imin((i64)u, avail);
            int end = out_end;
            int q = n_ent;
            if (w > 0) {
                end += w;
                const i64 delta = t_idx - out_end;
                if (delta < -(1ll << 30) || delta > (1ll << 30)) q = PLAN_MAXE + 1;
                else { put(q, T_TRACK, out_end, delta, 0); ++q; }
            }
            if (end < L && q <= PLAN_MAXE) { put(q, T_ZERO, end, 0, 0); ++q; }
            n_ent = q;
        }
        n_ent = rfl(n_ent);
        if (n_ent > PLAN_MAXE) ok = false;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int2 *const h = hdr + k * (i64)chunks;
    for (int c = lane; c < chunks; c += WAVE) {
        int2 v = {0, -1};
        const i64 lo = (i64)c * A.chunk_len, hi = lo + A.chunk_len;
        if (ok && n_ent > 0 && lo < L64) {
            // entries are in output order, the first one starts at 0: [first, last] = the last that starts at or in front of
            // the chunk's first value ... the last that starts in front of its end
            int first = 0, last = 0;
            for (int i = 0; i < n_ent; ++i) {
                const i64 o = outs[wave][i];
                if (o <= lo) first = i;
                if (o < hi) last = i;
            }
            v.x = first; v.y = last - first + 1;
        }
        h[c] = v;
    }
}

// src/intervals.rs:19-126.  One thread per output value: the value is that of the LAST
// interval (in order) that covers the position -- what sequential painting leaves behind.
// `pmax[c]` = max(ends[list start .. c]): a position no earlier interval reaches is 0.0 without
// walking back over the whole list (gaps between intervals are the common case).
struct PaintTile { u32 idx[2 * WAVE]; float cv[PAINT_TILE]; int ce[PAINT_TILE]; };     // start bitmap + prefix, candidate values / ends
struct PaintImage { u32 idx[PAINT_CHUNK]; float cv[PAINT_TILE]; };                      // the leftovers kernel's image of one chunk
struct PaintTodo { int flag; int n_c; i64 lo_c; };      // per (query, chunk): 0 = done, 1 = per-value kernel, 2 = image (candidates [lo_c, lo_c + n_c))

// "Later intervals overwrite earlier ones" = every position takes the candidate with the HIGHEST index
// that covers it: one wave paints candidate indices into an LDS image of the chunk with ds_max (order-free;
// lane = interval for short ones, the whole wave for a long one) and streams the image out through the
// candidates' values.
__device__ __forceinline__ void paint_image(PaintImage &T, const int lane, const i64 lo_c, const int n_c, const i64 qs,
                                            const i64 j0, const int clen, const int *itv_starts, const int *itv_ends,
                                            const float *itv_values, float *row) {
    {   // clear the image
        const u32x4_a4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < PAINT_CHUNK / (4 * WAVE); ++t) *reinterpret_cast<u32x4_a4 *>(&T.idx[4 * (t * WAVE + lane)]) = z;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int b = 0; b < n_c; b += WAVE) {
        const int i = b + lane;
        int s_rel = 0, w = 0;
        if (i < n_c) {
            i64 s64 = (i64)itv_starts[lo_c + i] - qs - j0, e64 = (i64)itv_ends[lo_c + i] - qs - j0;
            s64 = s64 < 0 ? 0 : s64;
            e64 = e64 > clen ? clen : e64;
            if (e64 > s64) { s_rel = (int)s64; w = (int)(e64 - s64); }
            T.cv[i] = itv_values[lo_c + i];
        }
        const u32 tag = (u32)(i + 1);
        const bool is_long = w > 32;
        // short intervals: lane = interval
        for (int t = 0; __builtin_amdgcn_ballot_w64(!is_long && t < w) != 0; ++t)
            if (!is_long && t < w) atomicMax(&T.idx[s_rel + t], tag);
        // long intervals: the whole wave paints one at a time
        u64 m_long = __builtin_amdgcn_ballot_w64(is_long);
        while (m_long) {
            const int l = __builtin_ctzll(m_long);
            m_long &= m_long - 1;
            const int ls = rdl(s_rel, l), lw = rdl(w, l);
            const u32 lt = (u32)(b + l + 1);
            for (int t = lane; t < lw; t += WAVE) atomicMax(&T.idx[ls + t], lt);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int t = 0; t < PAINT_CHUNK / TRIP; ++t) {
        const int p = t * TRIP + GROUP * lane;
        if (p < clen) {
            const u32x4_a4 ix = *reinterpret_cast<const u32x4_a4 *>(&T.idx[p]);
            const float v0 = ix.x ? T.cv[ix.x - 1] : 0.0f, v1 = ix.y ? T.cv[ix.y - 1] : 0.0f;
            const float v2 = ix.z ? T.cv[ix.z - 1] : 0.0f, v3 = ix.w ? T.cv[ix.w - 1] : 0.0f;
            if (p + GROUP <= clen) {
                store_f32x4_wb(row + p, v0, v1, v2, v3);
            } else {
                if (p < clen) row[p] = v0;
                if (p + 1 < clen) row[p + 1] = v1;
                if (p + 2 < clen) row[p + 2] = v2;
            }
        }
    }
}


// values [j_begin, j_end) (step j_step) of query q, one thread per value: binary search + walk-back, cut short by
// the running maximum of ends where nothing covers the position
__device__ __forceinline__ void paint_values(const i64 j_begin, const i64 j_end, const i64 j_step, const i64 s0, const i64 e0,
                                             const i64 qs, const int *itv_starts, const int *itv_ends, const float *itv_values,
                                             const int *pmax, float *row) {
    for (i64 j = j_begin; j < j_end; j += j_step) {
        // c = last interval with start - qs <= j  (intervals are sorted by start)
        i64 lo = s0, hi = e0;   // first interval with start - qs > j
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if ((i64)itv_starts[mid] - qs <= j) lo = mid + 1; else hi = mid;
        }
        float v = 0.0f;
        if (lo > s0 && (i64)pmax[lo - 1] - qs > j) {
            for (i64 c = lo - 1; c >= s0; --c) {
                if ((i64)itv_ends[c] - qs > j) { v = itv_values[c]; break; }
            }
        }
        __builtin_nontemporal_store(v, row + j);
    }
}

// Two modes.  chunk_todo == NULL: the whole painting, grid (x, n_queries), a grid-stride loop over each row.
// chunk_todo != NULL (after the tiled kernel): only the chunks it left behind.  Almost every chunk is done by then,
// so a workgroup looks at 256 records at once (one per thread, grid = records / 256: 33 workgroups for cfg4 instead
// of 8 320) and works through the few that are flagged: 1 = per-value painting by the whole workgroup, 2 =
// overlapping candidates, wave 0 paints the chunk into the LDS image.
__global__ __launch_bounds__(256) void intervals_to_tracks_kernel(
    const i64 *offset_idxs, const int *starts, i64 starts_stride, i64 n_queries, const int *itv_starts,
    const int *itv_ends, const float *itv_values, const i64 *itv_offsets, const int *pmax, float *out,
    const i64 *out_offsets, int chunk_len, const PaintTodo *chunk_todo, i64 n_chunks, i64 list_div) {
    __shared__ PaintImage image;
    __shared__ int flags[256];
    if (!chunk_todo) {
        const i64 q = blockIdx.y;
        if (q >= n_queries) return;
        const i64 o0 = out_offsets[q];
        const i64 idx = offset_idxs[q] / list_div;
        paint_values((i64)blockIdx.x * blockDim.x + threadIdx.x, out_offsets[q + 1] - o0, (i64)gridDim.x * blockDim.x, itv_offsets[idx],
                     itv_offsets[idx + 1], starts[q * starts_stride], itv_starts, itv_ends, itv_values, pmax, out + o0);
        return;
    }
    const i64 total = n_chunks * n_queries;
    const i64 rec0 = (i64)blockIdx.x * 256;
    const int mine = rec0 + threadIdx.x < total ? chunk_todo[rec0 + threadIdx.x].flag : 0;
    flags[threadIdx.x] = mine;
    if (!__syncthreads_or(mine != 0)) return;
    for (int r = 0; r < 256; ++r) {
        const int flag = flags[r];              // (uniform)
        if (flag == 0) continue;
        const i64 rec = rec0 + r;
        const i64 q = rec / n_chunks, chunk = rec - q * n_chunks;
        const PaintTodo td = chunk_todo[rec];
        const i64 o0 = out_offsets[q];
        const i64 length = out_offsets[q + 1] - o0;
        const i64 idx = offset_idxs[q] / list_div;
        const i64 qs = starts[q * starts_stride];
        const i64 c0 = chunk * chunk_len;
        const i64 c1 = c0 + chunk_len < length ? c0 + chunk_len : length;
        if (flag == 2) {
            if (threadIdx.x < WAVE)
                paint_image(image, (int)threadIdx.x, td.lo_c, td.n_c, qs, c0, (int)(c1 - c0), itv_starts, itv_ends, itv_values,
                            out + o0 + c0);
        } else {
            paint_values(c0 + threadIdx.x, c1, blockDim.x, itv_offsets[idx], itv_offsets[idx + 1], qs, itv_starts, itv_ends,
                         itv_values, pmax, out + o0);
        }
        __syncthreads();                        // the image is reused by the next flagged chunk
    }
}

// Tiled painter: one wave per (query, 2048-value chunk).  The intervals that can touch the chunk
// are [lo_c, hi_c): hi_c = first start at or after the chunk's end, lo_c = first interval whose
// running max of ends passes the chunk's start (two interleaved 64-ary searches, 2 rounds for
// lists of thousands).  "Later intervals overwrite earlier ones" = every position takes the
// candidate with the HIGHEST index that covers it, so the wave paints candidate indices into an
// LDS image of the chunk with ds_max (order-free; lane = interval for short ones, the whole wave
// for a long one) and then streams the image out through the candidates' values.  Chunks with
// more than PAINT_TILE candidates are left to the per-value kernel above.
// Coarse per-list index (gvl_intervals_bucket_*): bucket b of list i covers positions
// [base[i] + 2048 b, base[i] + 2048 (b + 1)); lo[] = first interval whose running max of ends passes
// the bucket's start, hi[] = first interval that starts at or after the bucket's end (both relative
// to the list's first interval).  One lookup per chunk gives a SUPERSET of the chunk's candidates
// (intervals outside the chunk clip to nothing), instead of two dependent 64-ary searches.

__global__ __launch_bounds__(256) void intervals_to_tracks_tiled_kernel(
    const i64 *offset_idxs, const int *starts, i64 starts_stride, i64 n_queries, const int *itv_starts,
    const int *itv_ends, const float *itv_values, const i64 *itv_offsets, const int *pmax, float *out,
    const i64 *out_offsets, int chunk_len, int n_chunks, PaintTodo *chunk_todo, const PaintIndex X, const int force_image,
    int *complete_err, const i64 list_div) {      // non-NULL: the caller vouched that no chunk needs the leftovers launch (gvl_track_set.tile_complete)
    __shared__ PaintTile tiles[4];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    PaintTile &T = tiles[wave];
    __shared__ int probe_s[WAVE], probe_p[WAVE];
    const i64 q = blockIdx.y;
    const i64 chunk = (i64)blockIdx.x * 4 + wave;
    // (per-query values: scalar loads through the constant address space, see realign_tracks_kernel)
    typedef const int __attribute__((address_space(4))) *KInt;
    typedef const i64 __attribute__((address_space(4))) *KI64;
    // Three rounds, each requested as a whole before any of it is used (the asm statements name the values as scalar
    // operands: written value by value the compiler had put every load behind the use of the one before -- eight memory
    // round trips in a row in front of the first candidate record, and a chunk's wave is exactly that chain long):
    //   1. the query's output range, list number and first position,  2. the list's bounds and its bucket index's,
    //   3. (below) both bucket bounds;  then the candidate records.
    const i64 o0 = ((KI64)(u64)out_offsets)[q];
    const i64 o1 = ((KI64)(u64)out_offsets)[q + 1];
    const i64 idx_raw = ((KI64)(u64)offset_idxs)[q];
    const i64 qs = ((KInt)(u64)starts)[q * starts_stride];
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" :: "s"(o0), "s"(o1), "s"(idx_raw), "s"((int)qs));
#endif
    const i64 length = o1 - o0;
    const i64 idx = list_div == 1 ? idx_raw : idx_raw / list_div;
    const i64 s0 = ((KI64)(u64)itv_offsets)[idx], e0 = ((KI64)(u64)itv_offsets)[idx + 1];
    // (without a bucket index the three reads below land on the list's own bounds and are not used)
    const i64 *const xo = X.offsets ? X.offsets : itv_offsets;
    const i64 xb0 = ((KI64)(u64)xo)[idx], xb1 = ((KI64)(u64)xo)[idx + 1];
    const int xbase = ((KInt)(u64)(X.offsets && X.base ? X.base : (const int *)itv_offsets))[idx];
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" :: "s"(s0), "s"(e0), "s"(xb0), "s"(xb1), "s"(xbase));
#endif
    // the first round of both searches probes the same 64 strided entries of the query's list for
    // every chunk: wave 0 fetches them once for the block's 4 chunks
    if (!X.offsets && wave == 0 && e0 > s0) {
        const i64 st = (e0 - s0 + WAVE - 1) / WAVE;
        i64 pp = s0 + (i64)(lane + 1) * st - 1;
        if (pp > e0 - 1) pp = e0 - 1;
        probe_s[lane] = itv_starts[pp];
        probe_p[lane] = pmax[pp];
    }
    __syncthreads();
    if (chunk >= n_chunks) return;
    const i64 j0 = chunk * chunk_len;
    if (j0 >= length) { if (lane == 0 && chunk_todo) chunk_todo[q * n_chunks + chunk].flag = 0; return; }
    const i64 j1 = (length - j0 > chunk_len) ? j0 + chunk_len : length;
    // first start - qs >= j1 and first pmax - qs > j0: both searches advance together so that
    // their probe loads overlap (2 dependent rounds for lists of thousands instead of 4)
    i64 hi_c = 0, lo_c = 0;
    bool indexed = false;
    if (X.offsets) {
        const i64 b0 = xb0;
        const i64 nb = xb1 - b0;
        if (nb > 0) {
            const i64 base = xbase;
            i64 ba = (qs + j0 - base) >> 11, bb = (qs + j1 - 1 - base) >> 11;
            ba = ba < 0 ? 0 : (ba > nb - 1 ? nb - 1 : ba);
            bb = bb < 0 ? 0 : (bb > nb - 1 ? nb - 1 : bb);
            const int r_lo = ((KInt)(u64)X.lo)[b0 + ba], r_hi = ((KInt)(u64)X.hi)[b0 + bb];
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" :: "s"(r_lo), "s"(r_hi));
#endif
            lo_c = s0 + r_lo;
            hi_c = s0 + r_hi;
            if (lo_c > hi_c) lo_c = hi_c;
            indexed = hi_c - lo_c <= PAINT_TILE;
        }
    }
    if (!indexed) {
        i64 a1 = s0, b1 = e0, a2 = s0, b2 = e0;
        bool d1 = false, d2 = false;
        bool first = X.offsets == nullptr;      // (the shared first-round probes are only fetched without an index)
        while (!(d1 && d2)) {
            i64 p1 = 0, p2 = 0, st1 = 1, st2 = 1;
            int k1 = 0, k2 = 0;
            if (!d1) {
                if (a1 >= b1) d1 = true;
                else { st1 = (b1 - a1 + WAVE - 1) / WAVE; p1 = a1 + (i64)(lane + 1) * st1 - 1; if (p1 > b1 - 1) p1 = b1 - 1; k1 = first ? probe_s[lane] : itv_starts[p1]; }
            }
            if (!d2) {
                if (a2 >= b2) d2 = true;
                else { st2 = (b2 - a2 + WAVE - 1) / WAVE; p2 = a2 + (i64)(lane + 1) * st2 - 1; if (p2 > b2 - 1) p2 = b2 - 1; k2 = first ? probe_p[lane] : pmax[p2]; }
            }
            if (!d1) {
                const u64 m = __builtin_amdgcn_ballot_w64((i64)k1 - qs > j1 - 1);
                if (m == 0) { a1 = b1; d1 = true; }
                else {
                    const int f = __builtin_ctzll(m);
                    i64 pf = a1 + (i64)(f + 1) * st1 - 1; if (pf > b1 - 1) pf = b1 - 1;
                    if (st1 == 1) { b1 = pf; a1 = pf; d1 = true; }
                    else { if (f > 0) a1 += (i64)f * st1; b1 = pf; if (a1 >= b1) d1 = true; }
                }
            }
            if (!d2) {
                const u64 m = __builtin_amdgcn_ballot_w64((i64)k2 - qs > j0);
                if (m == 0) { a2 = b2; d2 = true; }
                else {
                    const int f = __builtin_ctzll(m);
                    i64 pf = a2 + (i64)(f + 1) * st2 - 1; if (pf > b2 - 1) pf = b2 - 1;
                    if (st2 == 1) { b2 = pf; a2 = pf; d2 = true; }
                    else { if (f > 0) a2 += (i64)f * st2; b2 = pf; if (a2 >= b2) d2 = true; }
                }
            }
            first = false;
        }
        hi_c = b1; lo_c = b2 < hi_c ? b2 : hi_c;
    }
    const i64 n_c64 = hi_c - lo_c;
    // (chunk_todo == NULL: a `tile_complete` interval set painted without the leftovers launch -- nobody reads the flags)
    PaintTodo *todo = chunk_todo ? chunk_todo + q * n_chunks + chunk : nullptr;
    if (n_c64 > PAINT_TILE) { if (lane == 0) { if (todo) todo->flag = 1; if (complete_err) *complete_err = 2; } return; }   // the per-value path takes it
    if (lane == 0 && todo) todo->flag = 0;
    const int n_c = (int)n_c64;
    const int clen = (int)(j1 - j0);
    float *row = out + o0 + j0;
    // ---- candidates that do not overlap (what a BigWig-like track is): no painting at all.  A start
    // BITMAP of the chunk (64 words) + its exclusive popcount prefix give, for any position, the number of
    // candidates that start at or before it -- i.e. the index of the only interval that can cover it --
    // with two LDS reads; its end says whether it does.  Overlapping candidates or equal starts take the
    // image path below (later intervals win: ds_max of candidate indices).
    {
        T.idx[lane] = 0u;                                     // bitmap: words 0..63, prefix: words 64..127
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        bool bad = force_image != 0;
        int n_before = 0;
        int carry_e = (int)0x80000000, carry_s = (int)0x80000000;          // end / start of the candidate in front
        // all candidate records are requested before the first one is used (<= 4 rounds of 64: one memory
        // round trip instead of one per round)
        int c_s[PAINT_TILE / WAVE], c_e[PAINT_TILE / WAVE]; float c_v[PAINT_TILE / WAVE];
        // (every lane of every round reads SOME candidate -- those behind the last one the last one again -- and does not use
        // it: a load under a predicate, or in a round that is skipped, is merged with a default value, and the merge
        // waits for it: one round trip per round again)
#pragma unroll
        for (int r_ = 0; r_ < PAINT_TILE / WAVE; ++r_) { c_s[r_] = 0; c_e[r_] = 0; c_v[r_] = 0.0f; }
        if (n_c > 0) {
#pragma unroll
            for (int r_ = 0; r_ < PAINT_TILE / WAVE; ++r_) {
                const int i = r_ * WAVE + lane;
                const i64 at = lo_c + (i < n_c ? i : n_c - 1);
                c_s[r_] = itv_starts[at]; c_e[r_] = itv_ends[at]; c_v[r_] = itv_values[at];
            }
        }
#pragma unroll
        for (int r_ = 0; r_ < PAINT_TILE / WAVE; ++r_) {
            const int b = r_ * WAVE;
            if (b >= n_c) break;
            const int i = b + lane;
            int sr = 0x7FFFFFFF, er = 0x7FFFFFFF;
            if (i < n_c) {
                i64 s64 = (i64)c_s[r_] - qs - j0, e64 = (i64)c_e[r_] - qs - j0;
                s64 = s64 < -(1ll << 30) ? -(1ll << 30) : (s64 > (1ll << 30) ? (1ll << 30) : s64);
                e64 = e64 < -(1ll << 30) ? -(1ll << 30) : (e64 > (1ll << 30) ? (1ll << 30) : e64);
                sr = (int)s64; er = (int)e64;
                T.ce[i] = er;
                T.cv[i] = c_v[r_];
            }
            int pe = __shfl_up(er, 1, WAVE), ps = __shfl_up(sr, 1, WAVE);
            if (lane == 0) { pe = carry_e; ps = carry_s; }
            if (i < n_c && (sr < pe || sr == ps)) bad = true;
            if (i < n_c && sr >= 0 && sr < clen) atomicOr(&T.idx[sr >> 5], 1u << (sr & 31));
            n_before += __builtin_popcountll(__builtin_amdgcn_ballot_w64(i < n_c && sr < 0));
            const int last = (n_c - b > WAVE ? WAVE : n_c - b) - 1;
            carry_e = rdl(er, last); carry_s = rdl(sr, last);
        }
        if (__builtin_amdgcn_ballot_w64(bad) == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const u32 wbits = T.idx[lane];
            const int cnt = __builtin_popcount(wbits);
            const int incl = wave_scan_inclusive<OpAdd>(cnt);
            T.idx[WAVE + lane] = (u32)(incl - cnt);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int base = n_before - 1;
#pragma unroll
            for (int t = 0; t < PAINT_CHUNK / TRIP; ++t) {
                const int p = t * TRIP + GROUP * lane;
                if (p < clen) {
                    const u32 wd = T.idx[p >> 5];
                    const int pre = base + (int)T.idx[WAVE + (p >> 5)];
                    const int bp = p & 31;                      // (a multiple of 4: the 4 positions share the word)
                    float v[GROUP];
                    const int i0 = pre + __builtin_popcount(wd & (0xFFFFFFFFu >> (31 - bp)));
                    const int i3 = pre + __builtin_popcount(wd & (0xFFFFFFFFu >> (28 - bp)));
                    if (i0 == i3) {
                        const int e0_ = i0 >= 0 ? T.ce[i0] : 0;
                        const float c0 = i0 >= 0 ? T.cv[i0] : 0.0f;
#pragma unroll
                        for (int g = 0; g < GROUP; ++g) v[g] = e0_ > p + g ? c0 : 0.0f;
                    } else {
#pragma unroll
                        for (int g = 0; g < GROUP; ++g) {
                            const int ig = pre + __builtin_popcount(wd & (0xFFFFFFFFu >> (31 - bp - g)));
                            v[g] = (ig >= 0 && T.ce[ig] > p + g) ? T.cv[ig] : 0.0f;
                        }
                    }
                    if (p + GROUP <= clen) {
                        store_f32x4_wb(row + p, v[0], v[1], v[2], v[3]);
                    } else {
                        row[p] = v[0];
                        if (p + 1 < clen) row[p + 1] = v[1];
                        if (p + 2 < clen) row[p + 2] = v[2];
                    }
                }
            }
            return;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // overlapping candidates or equal starts: the leftovers kernel paints this chunk into an LDS image
    if (lane == 0) { if (todo) { todo->flag = 2; todo->n_c = n_c; todo->lo_c = lo_c; } if (complete_err) *complete_err = 2; }
}

// bucket counts of every list (written at counts[i + 1] for the scan) and the list's base position
__global__ __launch_bounds__(256) void bucket_counts_kernel(const int *itv_starts, const i64 *itv_offsets, i64 n_lists,
                                                             i64 *counts, int *base) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) counts[0] = 0;
    if (i >= n_lists) return;
    const i64 s0 = itv_offsets[i], e0 = itv_offsets[i + 1];
    i64 n = 0;
    int b = 0;
    if (e0 > s0) {
        b = itv_starts[s0];
        n = ((i64)itv_starts[e0 - 1] - (i64)b) / PAINT_CHUNK + 1;
    }
    counts[i + 1] = n;
    base[i] = b;
}

__global__ __launch_bounds__(256) void bucket_fill_kernel(const int *itv_starts, const int *pmax, const i64 *itv_offsets,
                                                           i64 n_lists, const i64 *bkt_offsets, const int *base, int *lo_out,
                                                           int *hi_out) {
    const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= bkt_offsets[n_lists]) return;
    i64 a = 0, b = n_lists;                      // list i with bkt_offsets[i] <= g < bkt_offsets[i + 1]
    while (b - a > 1) {
        const i64 m = (a + b) >> 1;
        if (bkt_offsets[m] <= g) a = m; else b = m;
    }
    const i64 i = a;
    const i64 s0 = itv_offsets[i], e0 = itv_offsets[i + 1];
    const i64 x0 = (i64)base[i] + (g - bkt_offsets[i]) * PAINT_CHUNK, x1 = x0 + PAINT_CHUNK;
    i64 l = s0, h = e0;                          // first c with pmax[c] > x0
    while (l < h) { const i64 m = (l + h) >> 1; if ((i64)pmax[m] > x0) h = m; else l = m + 1; }
    lo_out[g] = (int)(l - s0);
    l = s0; h = e0;                              // first c with start >= x1
    while (l < h) { const i64 m = (l + h) >> 1; if ((i64)itv_starts[m] >= x1) h = m; else l = m + 1; }
    hi_out[g] = (int)(l - s0);
}

// pmax[c] = max(ends[s .. c]) within each queried list: one wave per list, 64 entries per trip
__global__ __launch_bounds__(256) void intervals_prefix_max_kernel(const i64 *list_idxs, i64 n_lists,
                                                                    const int *itv_ends, const i64 *itv_offsets,
                                                                    int *pmax) {
    const int lane = threadIdx.x & (WAVE - 1);
    for (i64 w = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < n_lists; w += ((i64)gridDim.x * blockDim.x) >> 6) {
        const i64 idx = list_idxs ? list_idxs[w] : w;
        const i64 s0 = itv_offsets[idx], e0 = itv_offsets[idx + 1];
        int carry = (int)0x80000000;
        for (i64 b = s0; b < e0; b += WAVE) {
            const i64 c = b + lane;
            int v = c < e0 ? itv_ends[c] : (int)0x80000000;
            // inclusive max scan (signed): bias to unsigned order for OpMaxU
            int u = wave_scan_inclusive<OpMaxU>((int)((u32)v ^ 0x80000000u));
            int m = (int)((u32)u ^ 0x80000000u);
            m = m > carry ? m : carry;
            if (c < e0) pmax[c] = m;
            carry = rdl(m, WAVE - 1);
        }
    }
}


