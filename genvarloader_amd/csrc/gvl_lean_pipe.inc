// gvl_lean_pipe.inc -- recon_lean_rows_kernel: the lean kernel's one-chunk form as a SOFTWARE PIPELINE over rows
// (included by gvl_hip.hip inside its anonymous namespace, behind gvl_lean.inc).
//
// Why.  recon_lean_kernel gives every row its own wave: request entries -> {slot line, contig bounds} -> window
// (three dependent memory levels, 3-4 us when they come from HBM) and THEN 8 KiB of one-hot stores.  A wave never
// has its reads and its stores in flight together, so a launch -- and a queue of launches, and one grid over sixteen
// batches (tools/exp_grid.py: 8.35 us per 4096 rows whatever the grid) -- runs at
// wave slots / (head + stores), not at the memory system's rate.  Here a wave takes rows w, w + W, w + 2 W, ... of the
// launch (W = waves in the grid) and keeps the NEXT row's window + slot line and the row-after-next's request entries
// in flight while it plans and stores the row in hand.
//
// How, on gfx950.  `vmcnt` retires in issue order, loads and stores alike: a load issued behind a row's stores is
// only usable once those stores have been acknowledged, and the compiler's own wait counts merge to vmcnt(0) across
// a loop's back edge.  So the prefetch does not go through registers at all: it is LDS-DMA (global_load_lds_dword /
// _dwordx4, inline asm -- no VGPR destination the compiler could copy or spill before the data has landed) into
// per-wave LDS buffers, issued at the TOP of a row's iteration, i.e. in front of that row's stores, and waited for at
// the iteration's end with a counted `s_waitcnt vmcnt(N)`, N = the store instructions issued behind the prefetch.
// A wave's stores are then never waited for before the wave's last row.  Per row three DMA instructions:
//   E  lanes 0..5 (RAG: 0..9): the row's request entries {contig, start, shift, geno_offset_idx lo / hi, to_rc's aligned
//      dword, RAG: out_offsets[k] and [k + 1]} from their arrays into 24 / 40 bytes of LDS (two rows ahead);
//   W  lanes 0..7: the 128-byte slot line + lanes 8..63: the first 896 bytes of the packed reference from the 16-byte line
//      IN FRONT of the one that holds the row's first base (a run behind an insertion near the row's start reads to the
//      left); then as many 16-byte lanes as the row needs of the rest (its bases, LEAN_TAIL more for deletions) (one row ahead).
// The row in hand then runs recon_lean_kernel's plan (src/reconstruct/mod.rs:85-198 restated on the record lanes)
// and phases A / B / C from LDS: phase A picks every lane's 8 bases at its run's offset out of the raw window (a row of
// one run: one ds_read2 + v_alignbit per step; a row with indels: two picks and a nibble mask; a lane whose 8 bases hold
// two allele starts: base by base) and writes the row back IN PLACE at offset 0.  Allele bytes behind an insertion's first
// byte come through SCALAR loads (lgkmcnt, not vmcnt: they can be waited for without waiting for the prefetch behind them).
//
// RAG (rows at out_offsets: ragged output, the reference's default, src/ffi/mod.rs:794-815; or a caller's plan): rows of
// any length up to 10 trips at any base offset; the stream stores whole 4-base groups at 4-byte-aligned addresses and the
// last 1-3 bases one by one.
//
// Rows this path does not take -- lead / trail padding, coordinates >= 2^30, unsorted or more than 64 records, no fixed
// point, runs that leave the fetched window (more than LEAN_TAIL deleted bases in front of a base), RAG rows longer than
// 10 trips, bytes-writing rows with a byte that is neither ACGT nor N -- are only MARKED in the loop (no stores) and run
// at the wave's end through the all-purpose body (lean_solo_rows; its LDS aliases the wave's own buffers, free by
// then), so that the streaming loop holds no call and the callee needs nothing of the caller's state.  Each costs its
// launch ~10 us of tail: BASELINE config 3 has none (tools/pipe_deferred.py).
//
// One grid over several batches (gvl_reconstruct_many; the loader's group): row k of the launch belongs to batch
// k / rows_per_batch, whose request arrays and outputs sit in a table behind the arguments (LeanMany, in the kernarg
// segment); fetching a row's table entry is a scalar-cache hit a row ahead of its use, not on anyone's critical path.

struct LeanBatch {
    const int *regions; const int *shifts; const i64 *geno_offset_idx; const u8 *to_rc;
    u8 *onehot; u8 *haps; i64 *out_offsets_w; i64 n_rows;
    const i64 *out_offsets;     // RAG launches: where the batch's rows start (gvl_hap_offsets / the caller's plan); NULL otherwise
    const u8 *keep; const i64 *keep_offsets;      // the batch's keep mask (both or neither): row kl's bytes at keep[keep_offsets[kl] ..]
    int *av; int *ap;           // ANN launches: the batch's annotation outputs (annot_v_idxs, annot_ref_pos)
    i64 max_row_len;            // RAG launches: THIS batch's bound on its longest row (the caller's; a longer row is written, and reported)
};
struct LeanMany { LeanBatch b[GVL_MANY_MAX]; };
static_assert(sizeof(LeanBatch) == 112, "indexed in the kernarg segment");
static_assert(sizeof(ReconArgs) % 8 == 0, "LeanMany follows ReconArgs in the kernarg segment");

// A wave's buffer: [slot line, 128 B][window: WINB bytes of the packed reference from the window's 16-byte-aligned start], twice,
// and the request entries of two rows.  Fixed-length launches: rows of at most 8 trips (2048 bases); RAG (rows at
// out_offsets, any length up to 10 trips = 2560 bases -- the reference's default ragged output of 2 kb regions): 10.
constexpr int PIPE_SLOT_BYTES = 16 * GVL_SLOT_RECS;
constexpr int PIPE_DMA1_WIN = 1024 - PIPE_SLOT_BYTES;            // window bytes the first DMA instruction brings (lanes 8..63)
// ragged rows: the bases in front of the output's first boundary of this many bases (4 bytes of one-hot / annotation each) go out one
// per lane, the body in groups counted from that boundary.  32 bases = 128 bytes: measured against 16 (profiles/r05_ragged_align.txt),
// rows of 2064 bases -- starts a multiple of 64 bytes but not of 128 -- cost 169 ns per MB of one-hot instead of 181, rows of 2052
// 184 instead of 195, rows that start on 128 bytes the same 167-171.
#ifndef GVL_RAG_HEAD
#define GVL_RAG_HEAD 32
#endif
constexpr int RAG_HEAD = GVL_RAG_HEAD;
static_assert(RAG_HEAD == 16 || RAG_HEAD == 32, "a head base per lane, the tail's three behind them");
template <bool RAG> struct PipeCfg {
    static constexpr int MAXT = RAG ? PIPE_RAG_MAXT : LEAN_MAX_TRIPS;        // trips of 256 bases per row
    static constexpr int STEPS = (MAXT + 1) / 2;                  // phase A: 512 bases per step
    static constexpr int WINB = RAG ? 1360 : 1104;
    static constexpr int BUFB = PIPE_SLOT_BYTES + WINB;
    static constexpr int ENT = 16;                                // request entries of a row: 6, RAG + 4 (its two offsets), a keep mask's two offsets + 4
};
// (ANN: + the slot records' variant indices, two rows of them; and room for the all-purpose body's annotated tables, which alias the wave's buffers at its end)
template <bool RAG, bool ANN = false> struct __attribute__((aligned(16))) PipeWaveT {
    u32 buf[2][PipeCfg<RAG>::BUFB / 4]; u32 ent[2][PipeCfg<RAG>::ENT]; u32 kp[2][4];
    u32 vid[ANN ? 2 : 1][ANN ? GVL_SLOT_RECS : 4];
    u32 room[ANN ? (sizeof(SoloLds<true>) + 3) / 4 - 2 * (PipeCfg<RAG>::BUFB / 4) : 4];
};
static_assert(sizeof(PipeWaveT<false>) >= sizeof(SoloLds<false>), "lean_solo_rows' tables alias the wave's buffers");
static_assert(sizeof(PipeWaveT<false, true>) >= sizeof(SoloLds<true>) && sizeof(PipeWaveT<true, true>) >= sizeof(SoloLds<true>), "... the annotated ones too");
// (the window starts 16 .. 31 bytes in FRONT of the row's first base: a run behind an insertion near the row's start reads to the left)
static_assert(GVL_REF4_PAD >= (LEAN_TAIL + 16 + 1) / 2 + 32, "what a window reads behind the row's last base stays inside ref4's padding");
static_assert(63 + PipeCfg<false>::MAXT * TRIP + LEAN_TAIL + 8 + 8 <= 2 * PipeCfg<false>::WINB, "alignment slack + row + tail + pick8's second dword");
static_assert(63 + PipeCfg<true>::MAXT * TRIP + LEAN_TAIL + 8 + 8 <= 2 * PipeCfg<true>::WINB, "alignment slack + row + tail + pick8's second dword");
static_assert(PipeCfg<true>::WINB <= PIPE_DMA1_WIN + 1024, "two DMA instructions bring a window");

// Diagnostic builds (-DGVL_DIAG) with gvl_diag_set_stamps and stamps[63] == 1: a TIMELINE of the pipelined kernel -- behind the 64 counters
// 16 u64 per row of the launch, s_memrealtime (100 MHz) at: 0 the wave's start (its first row only), 1 tables built, 2 first window landed,
// 3 top of the row's iteration (the next row's prefetch not yet issued), 4 records decoded / plan starts, 5 phase A starts, 6 phase B
// starts, 7 phase C starts, 8 stores issued, 9 the iteration's closing wait is over; 10 = the row's index in its wave (tools/stamps_pipe.py)
#ifdef GVL_DIAG
#define PIPE_STAMP(k, i) do { if (tl_on && lane == 0) RA.stamps[64 + (i64)(k) * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define PIPE_STAMP_N(k, i) do { PIPE_STAMP(k, i); if (tl_on) ++n_after; } while (0)
#else
#define PIPE_STAMP(k, i) do { } while (0)
#define PIPE_STAMP_N(k, i) do { } while (0)
#endif
typedef const LeanArgs __attribute__((address_space(4))) *LeanArgsK;
typedef const LeanBatch __attribute__((address_space(4))) *LeanBatchK;
typedef void __attribute__((address_space(3))) *PipeWaveLds;

// LDS-DMA: lane l's 4 / 16 bytes at `gsrc` land at LDS byte address lds_dst + 4 l / 16 l (lds_dst wave-uniform).  M0 is the
// compiler's: saved and restored inside the statement that uses it (cdna_hip_programming.md, "What hipcc does not do").
__device__ __forceinline__ void glds_b32(const void *gsrc, const u32 lds_dst) {
#if defined(__HIP_DEVICE_COMPILE__)
    u32 keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
#endif
}
__device__ __forceinline__ void glds_b128(const void *gsrc, const u32 lds_dst) {
#if defined(__HIP_DEVICE_COMPILE__)
    u32 keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
#endif
}
// wait until at most `n` of the wave's vector-memory operations are outstanding (the n youngest: issue order); counts above 32
// wait for all but 32 (fewer left outstanding = a stricter wait, never a weaker one)
__device__ __forceinline__ void wait_vm_all_but(const int n) {
#define GVL_WVM(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    switch (n < 0 ? 0 : (n > 32 ? 32 : n)) {
        GVL_WVM(1) GVL_WVM(2) GVL_WVM(3) GVL_WVM(4) GVL_WVM(5) GVL_WVM(6) GVL_WVM(7) GVL_WVM(8)
        GVL_WVM(9) GVL_WVM(10) GVL_WVM(11) GVL_WVM(12) GVL_WVM(13) GVL_WVM(14) GVL_WVM(15) GVL_WVM(16)
        GVL_WVM(17) GVL_WVM(18) GVL_WVM(19) GVL_WVM(20) GVL_WVM(21) GVL_WVM(22) GVL_WVM(23) GVL_WVM(24)
        GVL_WVM(25) GVL_WVM(26) GVL_WVM(27) GVL_WVM(28) GVL_WVM(29) GVL_WVM(30) GVL_WVM(31) GVL_WVM(32)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef GVL_WVM
}

// The rows a wave of recon_lean_rows_kernel has marked, run through the all-purpose body (SOLO) one after the other.
// Never returns (the wave ends here).  `mask` bit i = row w_raw + i * n_waves of the launch.
// crew_row0 >= 0 (round 6; RAG launches whose longest row is beyond PIPE_RAG_MAXT trips -- a spliced batch's few long exons among
// thousands of short ones): the wave belongs to one of the launch's FRONT workgroups (LeanArgs.front: one per 256 rows, dispatched
// before every other workgroup).  Each of its threads looks at one row's two offsets; the rows longer than the streaming loop takes are
// then run by the workgroup's four waves CHUNK BY CHUNK IN PARALLEL (chunk c of the crew's rows to wave c mod 4, counted over the
// rows), from the launch's first microsecond -- instead of one after the other, chunk after chunk, at the end of whichever wave met
// the row (a 6 000-base row: three chunks of the all-purpose body = 30 us behind a launch that is otherwise done in 40).  The streaming
// waves skip those rows.  `wg_lds`: 32 bytes every wave of the workgroup can see (the waves' ballots meet there before any SoloLds is used).
template <bool OH, bool HAPS, bool CL = false, bool ANN = false, bool CREW = false>
__device__ __noinline__ __attribute__((noreturn)) void lean_solo_rows(
        const u64 kernarg, const int w_raw, const int n_waves, const u32 mask, const LutsLds luts_lds, const PipeWaveLds pw_lds,
        const int crew_row0 = -1, const PipeWaveLds wg_lds = nullptr) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // (no DMA of the loop may land in what is SoloLds from here on)
    Luts &luts = *(Luts *)luts_lds;
    SoloLds<ANN> &solo = *(SoloLds<ANN> *)(void *)pw_lds;
#if defined(__HIP_DEVICE_COMPILE__)
    const LeanArgs LA = *(LeanArgsK)(u64)rfl64((i64)kernarg);
    ReconArgs A = *(ReconArgsK)(u64)(rfl64((i64)kernarg) + (i64)sizeof(LeanArgs));
    const LeanBatchK tab = (LeanBatchK)(u64)(rfl64((i64)kernarg) + (i64)(sizeof(LeanArgs) + sizeof(ReconArgs)));
#else
    LeanArgs LA_ = LeanArgs(); LA_.rows_per_batch = 1; LA_.ploidy = 1;      // (the host pass only parses this body)
    const LeanArgs LA = LA_; ReconArgs A = ReconArgs(); const LeanBatch *tab = nullptr;
#endif
    const int lane = threadIdx.x & (WAVE - 1);
    if (A.stamps && lane == 0 && !CREW) {      // (gvl_diag_set_stamps: how many rows / waves come here -- tools/pipe_deferred.py)
        atomicAdd(reinterpret_cast<unsigned long long *>(A.stamps), (unsigned long long)__builtin_popcount((u32)rfl((int)mask)));
        atomicAdd(reinterpret_cast<unsigned long long *>(A.stamps) + 1, 1ull);
    }
    u64 *const stamps0 = A.stamps;
    A.stamps = nullptr;               // (the all-purpose body's own stamps are per workgroup of ITS grid)
    for (int b = lane; b < 256; b += WAVE) {                  // (the same values from every writer)
        const u32 d = onehot_dword((u32)b);
        luts.oh[b] = d;
        luts.oh_rc[b] = __builtin_bswap32(d);
        luts.comp[b] = (u8)comp_byte((u32)b);
    }
    // row k of the launch, chunks c_first, c_first + c_step, ... of it -> the row's chunk count
    auto do_row = [&](const int k, const int c_first, const int c_step) -> int {
        const int bi = (int)((u32)k / (u32)LA.rows_per_batch);
        const int kl = k - bi * LA.rows_per_batch;
        const LeanBatch LB = tab[bi];
        A.regions = LB.regions; A.shifts = LB.shifts; A.geno_offset_idx = LB.geno_offset_idx; A.to_rc = LB.to_rc;
        A.onehot = LB.onehot; A.haps = LB.haps; A.out_offsets_w = LB.out_offsets_w; A.n_rows = LB.n_rows;
        A.out_offsets = LB.out_offsets;
        A.keep = LB.keep; A.keep_offsets = LB.keep_offsets;
        if (ANN) { A.av = LB.av; A.ap = LB.ap; }
        // (rows at out_offsets: RAG launches; fixed-length launches: row kl at kl * fixed_len)
        const i64 row_base = LB.out_offsets ? rfl64(LB.out_offsets[kl]) : (i64)kl * A.fixed_len;
        const i64 row_len64 = LB.out_offsets ? rfl64(LB.out_offsets[kl + 1]) - row_base : A.fixed_len;
        const int row_len = row_len64 < 0 ? 0 : (row_len64 > 0x7FFFFF00ll ? 0x7FFFFF00 : (int)row_len64);
        // a row longer than the caller's max_row_len hint is written in full HERE (the chunk loop below), but the contract is the
        // all-purpose kernel's, whose grid is sized by the hint: report it the same way
        if (LB.out_offsets && (i64)row_len > LB.max_row_len && A.async_err && lane == 0) *A.async_err = 1;
        const int query = LA.ploidy_shift >= 0 ? (kl >> LA.ploidy_shift) : (int)((u32)kl / (u32)LA.ploidy);
        const int *reg = LB.regions + (i64)query * LA.regions_stride;
        const int l_c = rfl(reg[0]), l_start = rfl(reg[1]);
        const bool ref_only = LA.ref_only != 0;          // (gvl_get_reference's rows: no shifts, no genotype slots)
        const int l_shift = ref_only ? 0 : rfl(LB.shifts[kl]);
        const i64 l_oidx = ref_only ? 0 : rfl64(LB.geno_offset_idx[kl]);
        const bool rc = LB.to_rc != nullptr && rfl((int)LB.to_rc[kl]) != 0;
        const bool c_ok = (u32)l_c < (u32)LA.n_contigs;
        const bool o_ok = !ref_only && l_oidx >= 0 && l_oidx < LA.n_geno_offsets;
        const i64 c_s = rfl64(A.ref_offsets[c_ok ? l_c : 0]), c_e = rfl64(A.ref_offsets[(c_ok ? l_c : 0) + 1]);
        i64 o_s = 0; int n_var = 0;
        if (c_ok && o_ok) {
            o_s = rfl64(A.go_starts[l_oidx]);
            const i64 nv = rfl64(A.go_stops[l_oidx]) - o_s;
            n_var = nv < 0 ? 0 : (nv > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)nv);
            if (A.dbg & GVL_ABL(DBG_ABL_NO_VARIANTS)) n_var = 0;
        }
        if (lane == 0) {
            RowIn ri;
            ri.c_s = c_s; ri.R = c_e - c_s; ri.ref_start = l_start; ri.shift = l_shift;
            ri.o_s = o_s; ri.keep_off = (LB.keep && LB.keep_offsets) ? LB.keep_offsets[kl] : 0; ri.row_base = row_base;
            ri.k = kl; ri.n_var = n_var; ri.L = row_len; ri.rc = rc ? 1 : 0;
            ri.flags = (l_shift < 0 || l_shift >= (1 << 30)) ? 2 : 0;
            if (ref_only && l_start >= rfl(reg[2])) ri.flags |= 4;       // src/reference/mod.rs:16-18: start >= stop leaves the row as it is (zeros)
            solo.ri = ri;
        }
        wave_lds_fence();
#pragma unroll 1
        for (int c = c_first; (c == 0 && c_step == 1) || (i64)c * A.chunk_len < (i64)row_len; c += c_step) {       // (a RAG row may be longer than a chunk)
            recon_body<OH ? (CL ? OH_CL : OH_LC) : OH_NONE, HAPS, ANN, true>(A, nullptr, &solo, luts, 0, c);
            wave_lds_fence();
        }
        return (int)(((i64)row_len + A.chunk_len - 1) / A.chunk_len);
    };
    if constexpr (!CREW) {
#pragma unroll 1
        for (u32 m = (u32)rfl((int)mask); m; m &= m - 1) {
            const int i = __builtin_ctz(m);
            (void)do_row(rfl(w_raw) + i * rfl(n_waves), 0, 1);
        }
    } else {
        const int wave = rfl((int)(threadIdx.x >> 6));
        const int k_mine = crew_row0 + (int)threadIdx.x;
        bool is_long = false;
        if (k_mine < LA.n_rows) {
            const int bi = (int)((u32)k_mine / (u32)LA.rows_per_batch);
            const int kl = k_mine - bi * LA.rows_per_batch;
            const i64 *oo = tab[rfl(bi)].out_offsets;          // (a workgroup's 256 rows: one batch, or two where they meet)
            if (bi != rfl(bi)) oo = tab[bi].out_offsets;
            is_long = oo != nullptr && oo[kl + 1] - oo[kl] > (i64)PIPE_RAG_MAXT * TRIP;
        }
        const u64 mine = __builtin_amdgcn_ballot_w64(is_long);
        volatile u64 *const xch = reinterpret_cast<volatile u64 *>((void *)wg_lds);
        if (lane == 0) xch[wave] = mine;
        __syncthreads();
        u64 ms[LEAN_WAVES];
#pragma unroll
        for (int w = 0; w < LEAN_WAVES; ++w) ms[w] = (u64)rfl64((i64)xch[w]);
        __syncthreads();                                          // (read by every wave before any of them writes its SoloLds over it)
        if (stamps0 && wave == 0 && lane == 0) {                  // (diagnostics: rows the crews took)
            int n = 0;
#pragma unroll
            for (int w = 0; w < LEAN_WAVES; ++w) n += __builtin_popcountll(ms[w]);
            if (n) atomicAdd(reinterpret_cast<unsigned long long *>(stamps0) + 15, (unsigned long long)n);
        }
        int base = 0;
#pragma unroll 1
        for (int w = 0; w < LEAN_WAVES; ++w) {
#pragma unroll 1
            for (u64 m = ms[w]; m; m &= m - 1)
                base += do_row(crew_row0 + WAVE * w + (int)__builtin_ctzll(m), (wave - base) & (LEAN_WAVES - 1), LEAN_WAVES);
        }
    }
    __builtin_amdgcn_endpgm();
}

// RAG: rows at out_offsets[k] .. out_offsets[k + 1] (ragged output, output_length = -1: the reference's default, src/ffi/mod.rs:794-815;
// or a caller's splice plan), any length up to PipeCfg<true>::MAXT trips, row starts at any base: the request entries carry the two
// offsets, the stream stores whole 4-base groups at 4-byte-aligned addresses and the last 1-3 bases one by one.
// CL (fixed-length rows only): the one-hot output is channel-major, (rows, 4, L) -- what the reference's docs feed a model
// (docs/source/index.md:114-115 rearranges seqpro's (.., L, 4) to (.., 4, L)): a pair of nibbles looks up the two bases' flags for all
// four channels at once (8 bytes), two v_perm per channel put four bases' flags into a dword, and a lane stores 16 bases per channel
// plane -- every store instruction one contiguous KB of one plane.
// ANN (haplotype bytes + annotations, src/ffi/mod.rs:2237-2397): per output base the variant it comes from (-1: the reference) and
// its reference coordinate (an allele's bases: its variant's position) -- two i32 streams made from what the plan already holds per
// record lane (allele start / bytes written / position / the delta behind it) + the records' variant indices, which arrive with the
// slot line (gvl_static.slot_vidx: one more LDS-DMA of two lanes).
// KM: the launch may carry a keep mask or be gvl_get_reference's (ref_only); false = both compiled out (the plain rows of a dataset:
// what they cost each row -- two more entry lanes, the tests, 12 % more instructions per row -- is not paid by launches without them).
template <bool OH, bool HAPS, bool RAG, bool CL = false, bool ANN = false, bool KM = true>
__global__ __launch_bounds__(LEAN_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void recon_lean_rows_kernel(
        const LeanArgs A, const ReconArgs RA, const LeanMany M) {
    static_assert(!CL || (OH && !RAG), "channel-major one-hot: fixed-length rows");
    static_assert(!ANN || HAPS, "annotated haplotypes: bytes + the two annotation streams (+ a one-hot in either layout)");
    typedef PipeCfg<RAG> CFG;
    typedef PipeWaveT<RAG, ANN> PipeWave;
    // The launch's arguments are read where they are used, through a pointer the compiler cannot see through (re-made
    // opaque at the top of every row): kept in registers across the loop they do not fit the 72 SGPRs a wave has at 8
    // waves per SIMD (800 / 8 less the trap handler's 16), and a spilled SGPR costs a v_readlane -- a VALU slot -- per use.
#if defined(__HIP_DEVICE_COMPILE__)
    LeanArgsK ka = (LeanArgsK)(u64)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
#else
    const LeanArgs *ka = &A;
#endif

    __shared__ uint2 lut[OH ? 512 : 1];                  // as recon_lean_kernel's
    __shared__ unsigned short blut[HAPS ? 512 : 1];
    __shared__ PipeWave pw_all[LEAN_WAVES];
    __shared__ Luts solo_luts;

    const int tid = threadIdx.x;
    int lane = tid & (WAVE - 1);                     // (not const: made opaque at the top of every row, below)
    const int wave = rfl(tid >> 6);
    PipeWave &pw = pw_all[wave];
    // RAG launches with rows beyond the streaming loop's 10 trips: the front workgroups are the long rows' crews (lean_solo_rows)
    int front = 0;
    if constexpr (RAG) {
        front = ka->front;
        if ((int)blockIdx.x < front)
            lean_solo_rows<OH, HAPS, CL, ANN, true>((u64)__builtin_amdgcn_kernarg_segment_ptr(), 0, 0, 0u, (LutsLds)&solo_luts, (PipeWaveLds)(void *)&pw,
                                                    (int)blockIdx.x * LEAN_THREADS, (PipeWaveLds)(void *)&pw_all[0]);
    }
    const int n_waves = ((int)gridDim.x - front) * LEAN_WAVES;
    const int w_raw = ((int)blockIdx.x - front) * LEAN_WAVES + wave;
    int L = ka->L;
#ifdef GVL_DIAG
    const bool tl_on = RA.stamps != nullptr && RA.stamps[63] == 1;
#endif
    PIPE_STAMP(w_raw < ka->n_rows ? w_raw : 0, 0);
    const u32 pw_lds = (u32)rfl((int)(u32)(u64)(PipeWaveLds)(void *)&pw);
#if defined(__HIP_DEVICE_COMPILE__)
    const LeanBatchK tab = (LeanBatchK)(u64)((i64)(u64)__builtin_amdgcn_kernarg_segment_ptr() + (i64)(sizeof(LeanArgs) + sizeof(ReconArgs)));
#else
    const LeanBatch *tab = M.b;
#endif
    typedef const i64 __attribute__((address_space(4))) *KI64;

    // a row of the launch as (batch, row of the batch); the wave's next row is n_waves further on
    struct BK { int bi, kl; };
    const int adv_q = (int)((u32)n_waves / (u32)ka->rows_per_batch), adv_r = n_waves - adv_q * ka->rows_per_batch;
    auto advance = [&](const BK x) -> BK {
        BK y; y.bi = x.bi + adv_q; y.kl = x.kl + adv_r;
        if (y.kl >= ka->rows_per_batch) { y.kl -= ka->rows_per_batch; ++y.bi; }
        return y;
    };

    // ---- E: the request entries of row (bi, kl) into pw.ent[e] (lanes 0..5, one DMA instruction) ----
    auto issue_entries = [&](const BK r, const int e) {
        const int kl = r.kl;
        const auto lb = tab + r.bi;
        const int *const regions = lb->regions;
        const int *const shifts = lb->shifts;
        const i64 *const goi = lb->geno_offset_idx;
        const u8 *const to_rc = lb->to_rc;
        const int query = ka->ploidy_shift >= 0 ? (kl >> ka->ploidy_shift) : (int)((u32)kl / (u32)ka->ploidy);
        const u8 *p_reg = reinterpret_cast<const u8 *>(regions + (i64)query * ka->regions_stride);
        // (ref_only -- gvl_get_reference's rows: no shifts, no genotype slots; the "shift" entry carries the region's END instead)
        const u8 *p_shift = (KM && ka->ref_only) ? p_reg + 8 : reinterpret_cast<const u8 *>(shifts + kl);
        const u8 *p_oidx = (KM && ka->ref_only) ? p_reg : reinterpret_cast<const u8 *>(goi + kl);
        const u8 *pb = to_rc ? to_rc + kl : p_reg;                 // to_rc is a byte array: its byte's aligned dword
        const u8 *p_rc = pb - ((u32)(u64)pb & 3u);
        const u8 *src = lane == 0 ? p_reg : lane == 1 ? p_reg + 4 : lane == 2 ? p_shift : lane == 3 ? p_oidx : lane == 4 ? p_oidx + 4 : p_rc;
        if constexpr (RAG) {       // lanes 6..9: out_offsets[kl], out_offsets[kl + 1]
            const u8 *p_oo = reinterpret_cast<const u8 *>(lb->out_offsets + kl);
            src = lane >= 6 ? p_oo + 4 * (lane - 6) : src;
        }
        // a keep mask (src/reconstruct/mod.rs:86-90: the exonic mask of spliced haplotypes, src/genotypes/mod.rs:132-176): lanes
        // KE .. KE + 3 = keep_offsets[kl], keep_offsets[kl + 1] (batches without one: any readable address, the values are not used)
        constexpr int KE = RAG ? 10 : 6;
        const i64 *const kofs = KM ? lb->keep_offsets : nullptr;
        const u8 *p_ko = kofs ? reinterpret_cast<const u8 *>(kofs + kl) : p_reg - 4 * KE;
        src = lane >= KE ? p_ko + 4 * (lane - KE) : src;
        if (lane < KE + (kofs ? 4 : 0)) glds_b32(src, pw_lds + (u32)(offsetof(PipeWave, ent) + 4 * CFG::ENT * e));
    };

    // the state of a row between the moment its window is requested and the moment it is written
    struct Row { int kl; bool ok, rc; u32 G0, cs32; int o_win, R, l_start, l_shift, L; i64 l_oidx, base; u8 *onehot, *haps; const u8 *keep_row; int *av, *ap; };
    // lane l holds contig l's start (as a position of the packed reference) and length, -1 = not a contig the lean path takes
    // (a row's own are a readlane away); datasets with 64 contigs or more read them per row
    const bool ro_lanes = ka->n_contigs < WAVE;
    int ro_cs = 0, ro_len = -1;
    if (ro_lanes && lane < ka->n_contigs) {
        const i64 s0 = ka->ref_offsets[lane], s1 = ka->ref_offsets[lane + 1];
        ro_cs = (int)(u32)(u64)s0;
        ro_len = (s1 - s0 >= 0 && s1 - s0 < (1ll << 31)) ? (int)(s1 - s0) : -1;
    }

    // ---- W: decode row (bi, kl)'s entries (pw.ent[e], landed) and request its window + slot line into pw.buf[bf] ----
    auto issue_window = [&](const BK rk, const int e, const int bf) -> Row {
        Row r;
        r.kl = rk.kl;
        const auto lb = tab + rk.bi;
        const u8 *const to_rc = lb->to_rc;
        r.onehot = lb->onehot; r.haps = lb->haps;
        r.av = ANN ? lb->av : nullptr; r.ap = ANN ? lb->ap : nullptr;
        i64 *const oow = lb->out_offsets_w;
        const int n_rows_b = (int)lb->n_rows;
        const u32 ev = lane < (RAG ? 14 : 10) ? pw.ent[e][lane] : 0u;
        const int l_c = rdl((int)ev, 0);
        r.l_start = rdl((int)ev, 1); r.l_shift = rdl((int)ev, 2);
        i64 l_oidx = (i64)(((u64)(u32)rdl((int)ev, 4) << 32) | (u32)rdl((int)ev, 3));
        const bool ref_only = KM && ka->ref_only != 0;
        const int l_end = r.l_shift;                     // (ref_only: what the entry holds)
        if (ref_only) { r.l_shift = 0; l_oidx = 0; }
        const u32 l_rcw = (u32)rdl((int)ev, 5);
        const u32 rc_mis = ((u32)(u64)to_rc + (u32)r.kl) & 3u;
        r.rc = to_rc != nullptr && ((l_rcw >> (8u * rc_mis)) & 0xFFu) != 0;
        const bool c_ok = (u32)l_c < (u32)ka->n_contigs;
        const int cc = c_ok ? l_c : 0;
        if (ro_lanes) {
            r.cs32 = (u32)rdl(ro_cs, cc);
            r.R = rdl(ro_len, cc);
        } else {
            const i64 *p_ro = ka->ref_offsets + cc;
            const i64 c_s = ((KI64)(u64)p_ro)[0], c_e = ((KI64)(u64)p_ro)[1];
            r.cs32 = (u32)(u64)c_s;
            r.R = (c_e - c_s >= 0 && c_e - c_s < (1ll << 31)) ? (int)(c_e - c_s) : -1;
        }
        const bool o_ok = ref_only || (l_oidx >= 0 && l_oidx < ka->n_geno_offsets);
        r.l_oidx = l_oidx;
        const int r0 = r.l_start + r.l_shift;
        // the row's place in the output: row kl of its batch at kl * L, or (RAG) where the entries say
        bool len_ok = true;
        if constexpr (RAG) {
            const i64 o0 = (i64)(((u64)(u32)rdl((int)ev, 7) << 32) | (u32)rdl((int)ev, 6));
            const i64 o1 = (i64)(((u64)(u32)rdl((int)ev, 9) << 32) | (u32)rdl((int)ev, 8));
            r.base = o0;
            len_ok = o1 - o0 > 0 && o1 - o0 <= (i64)CFG::MAXT * TRIP;       // (longer rows -- and empty ones -- are the all-purpose body's)
            // (... a long one, in a launch with front workgroups, is THEIRS: L = -1, neither streamed nor deferred by this wave)
            r.L = len_ok ? (int)(o1 - o0) : ((ka->front > 0 && o1 - o0 > (i64)CFG::MAXT * TRIP) ? -1 : 0);
        } else {
            r.base = (i64)r.kl * L;
            r.L = L;
        }
        // the lean path's rows: inside their contig, 30-bit coordinates, and the window readable without padding
        r.ok = c_ok && o_ok && len_ok && r.l_start >= 0 && r.l_start < (1 << 30) && r.l_shift >= 0 && r.l_shift < (1 << 30) &&
               r.R >= 0 && (i64)r0 + r.L <= (i64)r.R && !(ka->dbg & DBG_LEAN_SOLO);
        // (padded_slice, src/reference/mod.rs:9-50: start >= stop leaves the row untouched, a stop behind the contig pads: not this path's rows)
        if (ref_only) r.ok = r.ok && r.l_start < l_end && l_end <= r.R;
        r.G0 = r.cs32 + (u32)r0;
        // the window's first byte: the 16-byte line in FRONT of the one that holds the row's first base (32 .. 63 nibbles of slack:
        // the run behind an insertion of n bases near the row's start reads n bases to the left of where the row begins)
        u32 a0 = (r.G0 >> 1) & ~15u;
        a0 = a0 >= 16u ? a0 - 16u : a0;
        r.o_win = (int)(r.G0 - 2u * a0);
        if (!RAG && oow && lane == 0) {           // (RAG launches read their offsets, they do not write any)
            oow[r.kl] = r.base;
            if (r.kl == n_rows_b - 1) oow[r.kl + 1] = r.base + r.L;
        }
        // the row's keep bytes (at most the 8 of a slot line's records; a slot that overflows its line reads its own): the aligned
        // dwords that hold them -- every dword asked for holds at least one of the row's bytes, so none leaves their pages
        r.keep_row = nullptr;
        if (KM && lb->keep != nullptr && lb->keep_offsets != nullptr) {
            constexpr int KE = RAG ? 10 : 6;
            const i64 k0 = (i64)(((u64)(u32)rdl((int)ev, KE + 1) << 32) | (u32)rdl((int)ev, KE));
            const i64 k1 = (i64)(((u64)(u32)rdl((int)ev, KE + 3) << 32) | (u32)rdl((int)ev, KE + 2));
            r.keep_row = lb->keep + k0;
            const u32 mis = (u32)(u64)r.keep_row & 3u;
            i64 cnt = k1 - k0;
            cnt = cnt < 0 ? 0 : (cnt > GVL_SLOT_RECS ? GVL_SLOT_RECS : cnt);
            const int n_dw = (int)((mis + (u32)cnt + 3u) >> 2);
            if (r.ok && lane < n_dw) glds_b32(r.keep_row - mis + 4 * lane, pw_lds + (u32)(offsetof(PipeWave, kp) + 16 * bf));
        }
        if (ANN && r.ok && lane < 2)           // the slot records' variant indices: 8 x i32 = two 16-byte lanes
            glds_b128(reinterpret_cast<const u8 *>(ka->slot_vidx + (l_oidx * GVL_SLOT_RECS + 4 * lane)), pw_lds + (u32)(offsetof(PipeWave, vid) + 4 * GVL_SLOT_RECS * bf));
        if (r.ok) {
            // two DMA instructions: lanes 0..7 the slot line + lanes 8..63 the window's first 896 bytes; then what the row needs
            // of the rest (its own bases, LEAN_TAIL more for deletions, the slack of an unaligned start)
            const u32 dst = pw_lds + (u32)(offsetof(PipeWave, buf) + CFG::BUFB * bf);
            const u8 *win = ka->ref4 + a0;
            const u8 *s1 = lane < GVL_SLOT_RECS ? reinterpret_cast<const u8 *>(ka->srec + (l_oidx * GVL_SLOT_RECS + lane))
                                                : win + 16 * (lane - GVL_SLOT_RECS);
            if (lane < GVL_SLOT_RECS ? !ref_only : !(ka->dbg & GVL_ABL(DBG_ABL_NO_LOADS))) glds_b128(s1, dst);      // (ref_only: no slot line)
            const int need = (r.o_win + r.L + LEAN_TAIL + 16 + 1) >> 1;               // window bytes the row's picks may touch
            const int l2 = (need - PIPE_DMA1_WIN + 15) >> 4;                          // lanes of the second instruction
            if (lane < l2 && lane < (CFG::WINB - PIPE_DMA1_WIN) / 16 && !(ka->dbg & GVL_ABL(DBG_ABL_NO_LOADS))) glds_b128(win + PIPE_DMA1_WIN + 16 * lane, dst + 1024u);
        }
        return r;
    };

    // ---- prologue: entries of the wave's first row, tables while they are out, its window, the second row's entries ----
    const bool have0 = w_raw < ka->n_rows;
    BK bk0;
    bk0.bi = (int)((u32)w_raw / (u32)ka->rows_per_batch);
    bk0.kl = w_raw - bk0.bi * ka->rows_per_batch;
    if (have0) issue_entries(bk0, 0);
    {
        const int b = tid & 255;
        const u32 lo = nibble_onehot((u32)b & 15u), hi = nibble_onehot((u32)b >> 4);
        if (tid < 256) {
            if (OH && CL) {
                fill_cl_lut(lut, b, lo, hi);
            } else if (OH) {
                lut[b] = make_uint2(lo, hi);
                lut[256 + b] = make_uint2(__builtin_bswap32(hi), __builtin_bswap32(lo));
            }
            if (HAPS) {
                const u32 b0 = nibble_byte((u32)b & 15u), b1 = nibble_byte((u32)b >> 4);
                blut[b] = (unsigned short)(b0 | (b1 << 8));
                blut[256 + b] = (unsigned short)(comp_byte(b1) | (comp_byte(b0) << 8));
            }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // (LDS only: the DMA stays in flight)
    if (!have0) return;
    PIPE_STAMP(w_raw, 1);
    __builtin_amdgcn_s_setprio(3);
    // (everything has landed and the compiler knows it: a load its wait-count model believes may still be pending at the
    // loop's back edge costs every iteration a vmcnt(0) where its register is written or read next)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(ro_cs), "+v"(ro_len) :: "memory");
    Row nx = issue_window(bk0, 0, 0);
    BK bk_w = advance(bk0);                             // the row whose window goes out next
    int n_left = (ka->n_rows - 1 - w_raw) / n_waves;      // rows of this wave behind the one in hand
    if (n_left > PIPE_MAX_ROWS - 1) {                    // (the host sizes the grid for at most PIPE_MAX_ROWS rows per wave: never silently)
        n_left = PIPE_MAX_ROWS - 1;
        if (RA.async_err && lane == 0) *RA.async_err = 3;
    }
    if (n_left >= 1) issue_entries(bk_w, 1);
    BK bk_e = advance(bk_w);                            // the row whose entries go out next
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PIPE_STAMP(w_raw, 2);

    u32 solo_mask = 0;
#pragma unroll 1
    for (int it = 0; ; ++it, --n_left) {
#if defined(__HIP_DEVICE_COMPILE__)
        // (the lane number and the row length too: or every loop-invariant lane predicate -- "lane < 6", "this lane's 4 bases of trip
        // u lie inside the row", ... -- is hoisted into an SGPR pair of its own, and spilled)
        asm volatile("" : "+s"(ka));
        asm volatile("" : "+v"(lane));                 // (its own statement: one VGPR output makes every output of a statement divergent)
#endif
        L = ka->L;
        const Row cur = nx;
#ifdef GVL_DIAG
        const int k_glob = w_raw + it * n_waves;
        if (tl_on && lane == 0) RA.stamps[64 + (i64)k_glob * 16 + 10] = (u64)it + 1;
#endif
        PIPE_STAMP(k_glob, 3);
        const int bf = it & 1;
        const bool more = n_left >= 1;
        // ---- prefetch, in front of everything this row stores: the next row's window + slot line (its entries have
        // landed), the row after that one's entries
        if (more) {
            nx = issue_window(bk_w, bf ^ 1, bf ^ 1);
            if (n_left >= 2) issue_entries(bk_e, bf);
            bk_w = bk_e;
            bk_e = advance(bk_e);
        }
        int n_after = 0;                                 // vector-memory instructions this iteration issues behind the prefetch

        // ================= the row in hand (recon_lean_kernel's one-chunk form, from LDS) =================
        const int k = cur.kl;
        u32 *const row = pw.buf[bf] + PIPE_SLOT_BYTES / 4; // the raw window; from phase A on: the row as nibbles in output coordinates
        const int Lr = RAG ? (cur.L < 0 ? 0 : cur.L) : L;                  // this row's length
        const u32 G0 = cur.G0, cs32 = cur.cs32;
        const i64 R64 = (i64)cur.R;
        const int l_start = cur.l_start, l_shift = cur.l_shift;
        const int r0 = l_start + l_shift;
        const bool rc = cur.rc;
        bool lean_row = cur.ok;
        int why = lean_row ? 0 : 1;                      // (diagnostics: why a row is deferred)
        const int q_lane = 8 * lane;

        i32x4 rec = {0, 0, (int)GVL_SREC_EMPTY, 0};
        if (lean_row && lane < GVL_SLOT_RECS && !(KM && ka->ref_only)) rec = *reinterpret_cast<const i32x4 *>(&pw.buf[bf][4 * lane]);
        int vid = -1;                                    // ANN: the record's variant index
        if (ANN && lean_row && lane < GVL_SLOT_RECS) vid = (int)pw.vid[ANN ? bf : 0][lane & (GVL_SLOT_RECS - 1)];
        int n_rec = GVL_SLOT_RECS;
        bool ovf_solo = false;
        if (lean_row && rfl(rec.z) == (int)GVL_SREC_OVERFLOW) {
            // a slot that overflows its line: up to 64 records from the CSR's inline records (ordinary loads, three dependent
            // levels: this wave waits for everything it has in flight -- 0.3 % of BASELINE config 3's rows; deferring them
            // instead made 2 % of the waves end 10-15 us late)
            ovf_solo = true;
            const gvl_grec *const grec = ka->grec;
            if (grec) {
                const i64 oidx = cur.l_oidx;
                const i64 o_s = ka->go_starts[oidx];
                const i64 nv = ka->go_stops[oidx] - o_s;
                if (nv >= 0 && nv <= WAVE) {
                    ovf_solo = false;
                    n_rec = (int)nv;
                    rec.x = 0; rec.y = 0; rec.z = (int)GVL_SREC_EMPTY; rec.w = 0;
                    if (lane < n_rec) {
                        rec = *reinterpret_cast<const i32x4 *>(grec + (o_s + lane));
                        const u32 ee = (u32)rec.z;
                        vid = rec.w;                     // (the inline records carry the variant index where the slot records carry the ALT offset)
                        rec.w = (ee >> 8) > 1u ? (int)(u32)(u64)ka->alt_offsets[rec.w] : 0;
                        // (used HERE: a load the compiler's wait-count model believes may still be pending at the loop's back
                        // edge costs every iteration a vmcnt(0) where its register is written next)
                        asm volatile("" : "+v"(rec.x), "+v"(rec.y), "+v"(rec.z), "+v"(rec.w));
                    }
                }
            }
        }
        const bool short_scans = n_rec <= 8;
        const u32 e = (u32)rec.z;
        // a record the row's keep mask drops does not take part in anything (src/reconstruct/mod.rs:86-90)
        bool kept = true;
        if (KM && cur.keep_row != nullptr) {
            if (n_rec <= GVL_SLOT_RECS) {
                const u32 bo = ((u32)(u64)cur.keep_row & 3u) + (u32)lane;
                const u32 dw = pw.kp[bf][(bo >> 2) & 3u];
                kept = lane >= GVL_SLOT_RECS || ((dw >> (8u * (bo & 3u))) & 0xFFu) != 0u;
            } else {
                u32 kb = lane < n_rec ? (u32)cur.keep_row[lane] : 1u;
                asm volatile("" : "+v"(kb));          // (landed before the loop goes on: see the note at the overflow path)
                kept = kb != 0u;
            }
        }
        const bool valid = lane < n_rec && e != GVL_SREC_EMPTY && e != GVL_SREC_OVERFLOW && kept;
        const int pos = rec.x, d = rec.y;
        int alen = (int)(e >> 8);
        const u32 inl = e & 0xFFu;
        const bool is_snp = d == 0 && alen == 1;
        const int pos_prev = dpp_mov<0x138, 0xf>(-1, pos);               // wave_shr:1
        const u64 m_bad = __builtin_amdgcn_ballot_w64(
            ovf_solo ||
            (valid && (pos < 0 || pos >= (1 << 30) || d <= -(1 << 30) || d >= (1 << 30) || alen >= 0xFFFFFF)) ||
            (lane > 0 && valid && pos < pos_prev));                        // (the scans below assume sorted positions)
        if (m_bad != 0) { if (lean_row) why = 2; lean_row = false; }
        const u64 m_plain = __builtin_amdgcn_ballot_w64((valid && (!is_snp || (i64)pos + 1 > R64)) || (lane > 0 && valid && pos == pos_prev));
        const int alen0 = alen;                          // (a shift may cut the allele below)
        const int altoff = rec.w;
        const u64 m_ins = lean_row ? __builtin_amdgcn_ballot_w64(valid && alen0 > 1) : 0;

        // ---- plan (src/reconstruct/mod.rs:85-198; recon_lean_kernel's, verbatim in what it computes) ----
        PIPE_STAMP_N(k_glob, 4);
        bool applied = false, nonsnp = false;
        int skip_l = 0, a_out = 0, w_i = 0;
        u32 dv = 0, d_init = G0;
        if (lean_row && m_plain == 0) {
            // SNPs only, distinct positions inside the contig: SNP i sits at pos_i - r0 iff that is inside the row
            a_out = pos - r0;
            applied = valid && pos >= r0 && a_out < Lr;
            w_i = 1;
        } else if (lean_row) {
            const int ref_start = l_start;
            int rem = l_shift;
            int ref_idx0 = ref_start;
            const int E = pos - (d < 0 ? d : 0) + 1;                              // v_ref_end, :96
            {   // DEL spanning the window start (:99-102): the last one in order sets ref_idx
                const u64 m_span = __builtin_amdgcn_ballot_w64(valid && pos < ref_start && d < 0 && E >= ref_start);
                if (m_span) ref_idx0 = rdl(E, 63 - __builtin_clzll(m_span));
            }
            bool cand = valid && pos >= ref_start;
            if (rem > 0) {      // shift consumption (:115-146)
                const int base = ref_idx0;
                const u64 m_t = __builtin_amdgcn_ballot_w64(cand && pos >= base && (pos - base) + alen >= rem);
                if (m_t == 0) {
                    cand = false;                       // the shift is still open after the last variant
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
                            if (lane == f) { alen -= skip; skip_l = skip; }
                        }
                    }
                    rem = 0;
                }
            }
            // first ALT wins (:108-110): fixed point of B = {i : pos_i >= max(ref_idx0, max E over B before i)}
            bool inB = cand;
            int PM = 0;
            {
                u64 mB = __builtin_amdgcn_ballot_w64(inB);
                bool stable = false;
#pragma unroll 1
                for (int r_ = 0; r_ < 4 && !stable; ++r_) {
                    PM = lean_scan_excl<OpMaxU>(inB ? E : 0, lane, short_scans);
                    PM = PM > ref_idx0 ? PM : ref_idx0;
                    inB = cand && pos >= PM;
                    const u64 m2 = __builtin_amdgcn_ballot_w64(inB);
                    stable = m2 == mB;
                    mB = m2;
                }
                if (!stable) { lean_row = false; why = 3; }
            }
            const int n_i = inB ? pos - PM : 0;
            const int S_i = inB ? OpSat::f(n_i, alen) : 0;
            const int X = lean_scan_excl<OpSat>(S_i, lane, short_scans);
            a_out = OpSat::f(X, n_i);
            applied = inB && a_out < Lr;                                           // :154-158 break
            w_i = applied ? ((alen < Lr - a_out) ? alen : Lr - a_out) : 0;         // :178
            nonsnp = applied && !is_snp;
            dv = cs32 + (u32)E - (u32)(a_out + alen);
            // the walk's state behind the last applied variant, then the tail (:200-255): it must reach Lr without padding
            int ref_idx_end = ref_idx0, out_idx_end = 0;
            const u64 m_app = __builtin_amdgcn_ballot_w64(applied);
            if (m_app) {
                const int last = 63 - __builtin_clzll(m_app);
                ref_idx_end = rdl(E, last);
                out_idx_end = rdl(a_out, last) + rdl(w_i, last);
            }
            if (rem > 0) {                            // the shift never completed: nothing was applied
                const i64 t = (i64)ref_idx0 + rem;
                ref_idx_end = (int)(t < R64 ? t : R64);
                d_init = cs32 + (u32)ref_idx_end;
            } else {
                d_init = cs32 + (u32)ref_idx0;
            }
            if (Lr - out_idx_end > 0 && (i64)(Lr - out_idx_end) > R64 - (i64)ref_idx_end) { lean_row = false; why = 4; }   // trailing pad
        }

        // ---- phase A: every lane's 8 bases per step out of the raw window, at its run's offset ----
        PIPE_STAMP_N(k_glob, 5);
        // Nibble n of the buffer = packed-reference position 2 a0 + n; output position q of a run with delta dd (position
        // q + dd) therefore sits at q + (dd - 2 a0).  A run's offset from the window's own (G0 - 2 a0 <= 31) is what its
        // indels moved it by: as in recon_lean_kernel it must lie in [0, LEAN_TAIL], and no two allele starts may share
        // a lane's 8 bases -- rows beyond that (recon_lean_kernel re-reads their runs from memory) are deferred.
        const u64 m_ns = __builtin_amdgcn_ballot_w64(nonsnp);
        const int o_win = cur.o_win;
        u32 x[CFG::STEPS];
        if (lean_row) {
            const int rho0 = (int)(d_init - G0);
            bool in_win = rho0 >= 0 && rho0 <= LEAN_TAIL && !((ka->dbg & DBG_NO_REALIGN_LDS) && m_ns != 0);
            if (m_ns == 0) {
                // ONE run: every lane's 8 bases sit at the same offset from the window's start
                const int off = rho0 + o_win;
                const u32 sh = 4u * ((u32)off & 7u);
                const u32 *const src = row + (off >> 3) + lane;
#pragma unroll
                for (int s = 0; s < CFG::STEPS; ++s) {
                    x[s] = 0;
                    if (s * 512 < Lr && in_win) x[s] = __builtin_amdgcn_alignbit(src[s * WAVE + 1], src[s * WAVE], sh);
                }
            } else {
                int rl[CFG::STEPS], rh[CFG::STEPS], cut[CFG::STEPS];
#pragma unroll
                for (int s = 0; s < CFG::STEPS; ++s) { rl[s] = rho0 + o_win; rh[s] = rho0 + o_win; cut[s] = 8; }
                u32 multis = 0;                              // steps in which this lane's 8 bases hold TWO allele starts: base by base, below
                for (u64 m = m_ns; m; m &= m - 1) {
                    const int j = __builtin_ctzll(m);
                    const int aj = rdl(a_out, j);
                    const int rho = (int)((u32)rdl((int)dv, j) - G0);
                    in_win = in_win && aj - 7 + rho + o_win >= 0 && rho <= LEAN_TAIL;
#pragma unroll
                    for (int s = 0; s < CFG::STEPS; ++s) {
                        const int q = s * 512 + q_lane;
                        if (q >= aj) { rl[s] = rho + o_win; rh[s] = rho + o_win; }
                        else if (aj <= q + 7) {
                            if (cut[s] != 8) multis |= 1u << s;
                            else cut[s] = aj - q;
                            rh[s] = rho + o_win;
                        }
                    }
                }
                auto pick8 = [&](const int r) -> u32 {
                    const u32 lo = row[r >> 3], hi = row[(r >> 3) + 1];
                    return __builtin_amdgcn_alignbit(hi, lo, 4u * ((u32)r & 7u));
                };
                const int lim = (2 * CFG::WINB) - 16;       // (lanes behind a short row's end, rows that are about to be deferred: stay inside the buffer)
#pragma unroll
                for (int s = 0; s < CFG::STEPS; ++s) {
                    x[s] = 0;
                    if (s * 512 < Lr) {
                        const int q = s * 512 + q_lane;
                        int a = q + rl[s], b = q + rh[s];
                        a = a < 0 ? 0 : (a > lim ? lim : a);
                        b = b < 0 ? 0 : (b > lim ? lim : b);
                        const u32 y = pick8(a);
                        const u32 z = pick8(b);
                        const u32 lowm = cut[s] >= 8 ? 0xFFFFFFFFu : ((1u << (4 * cut[s])) - 1u);
                        x[s] = (y & lowm) | (z & ~lowm);
                    }
                }
                if (__builtin_amdgcn_ballot_w64(multis != 0) && in_win) {
                    // two allele starts less than 8 bases apart (0.04 % of BASELINE config 3's rows; deferred, every one of them made
                    // its launch end 10 us late): those lanes find each of their 8 bases' run on its own, from the same window
#pragma unroll
                    for (int s = 0; s < CFG::STEPS; ++s) {
                        if (__builtin_amdgcn_ballot_w64((multis >> s) & 1u)) {
                            u32 v = 0;
#pragma unroll 1
                            for (int i = 0; i < 8; ++i) {
                                const int qq = s * 512 + q_lane + i;
                                int dd = rho0 + o_win;
                                for (u64 m = m_ns; m; m &= m - 1) {
                                    const int j = __builtin_ctzll(m);
                                    if (qq >= rdl(a_out, j)) dd = (int)((u32)rdl((int)dv, j) - G0) + o_win;
                                }
                                int idx = qq + dd;
                                idx = idx < 0 ? 0 : (idx > lim + 7 ? lim + 7 : idx);
                                v |= ((row[idx >> 3] >> (4u * ((u32)idx & 7u))) & 0xFu) << (4 * i);
                            }
                            if ((multis >> s) & 1u) x[s] = v;
                        }
                    }
                }
            }
            if (!in_win) { if (lean_row) why = 5; lean_row = false; }
        }
        if (__builtin_amdgcn_ballot_w64(lean_row) == 0) {                       // (lean_row is wave-uniform)
            if (!(RAG && cur.L < 0)) solo_mask |= 1u << it;
            if (RA.stamps && lane == 0) atomicAdd(reinterpret_cast<unsigned long long *>(RA.stamps) + 2 + why, 1ull);
        } else {
            wave_lds_fence();                                                   // every lane has read: write the row in place
#pragma unroll
            for (int s = 0; s < CFG::STEPS; ++s)
                if (s * 512 < Lr) row[s * WAVE + lane] = x[s];
            wave_lds_fence();

            // ---- phase B: SNPs and allele bytes ----
            PIPE_STAMP_N(k_glob, 6);
            if (applied && w_i > 0 && skip_l == 0) row_set_nibble(row, a_out, ref4_nibble(inl));      // an allele's first byte is inline
            for (u64 m = m_ins; m; m &= m - 1) {
                // byte i (>= 1) of variant j's allele lands at a_out_j + i - skip_j if the variant is applied and the byte is
                // among the w_j the row has room for.  The bytes come through SCALAR loads of their aligned dwords (up to 9:
                // 36 bytes; longer alleles by ordinary loads), lane t takes byte 1 + t.
                const int j = __builtin_ctzll(m);
                const int o_w = rdl(w_i, j), o_a = rdl(a_out, j), o_sk = rdl(skip_l, j);
                const int n_b = rdl(alen0, j) - 1;
                const u8 *src = ka->alt_alleles + ((u32)rdl(altoff, j) + 1u);
                const u32 mis = (u32)(u64)src & 3u;
                if (o_w > 0) {
                    if (mis + (u32)n_b <= 36u) {
                        typedef const u32 __attribute__((address_space(4))) *KU32;
                        const KU32 al = (KU32)(u64)(src - mis);
                        const int nd = (int)((mis + (u32)n_b + 3u) >> 2);
                        u32 sd[9];
#pragma unroll
                        for (int q = 0; q < 9; ++q) sd[q] = al[q < nd ? q : nd - 1];   // (never a dword behind the allele's last)
#if defined(__HIP_DEVICE_COMPILE__)
                        // (named as scalar registers: or the compiler folds "select one of two loaded dwords by lane" into ONE
                        // vector load from a per-lane address -- a vmcnt wait with the prefetch in flight behind it)
                        asm volatile("" : "+s"(sd[0]), "+s"(sd[1]), "+s"(sd[2]), "+s"(sd[3]), "+s"(sd[4]), "+s"(sd[5]), "+s"(sd[6]), "+s"(sd[7]), "+s"(sd[8]));
#endif
                        const u32 bo = mis + (u32)lane;
                        u32 dw = sd[0];
#pragma unroll
                        for (int q = 1; q < 9; ++q) dw = (bo >> 2) == (u32)q ? sd[q] : dw;
                        const u32 bv = (dw >> (8u * (bo & 3u))) & 0xFFu;
                        const int ii = 1 + lane - o_sk;
                        if (lane < n_b && ii >= 0 && ii < o_w) row_set_nibble(row, o_a + ii, ref4_nibble(bv));
                    } else {
                        for (int t0 = 0; t0 < n_b; t0 += WAVE) {
                            const int t = t0 + lane;
                            u32 bv = t < n_b ? (u32)src[t] : 0u;
                            asm volatile("" : "+v"(bv));          // (landed before the loop goes on: see the note at the overflow path)
                            const int ii = 1 + t - o_sk;
                            if (t < n_b && ii >= 0 && ii < o_w) row_set_nibble(row, o_a + ii, ref4_nibble(bv));
                        }
                    }
                }
            }
            wave_lds_fence();
            bool other_row = false;
            if (HAPS) {
                // a nibble 0 in the finished row = a byte that is neither ACGT nor N: only the byte reference can write it
                bool other = false;
#pragma unroll
                for (int s = 0; s < CFG::STEPS; ++s) {
                    if (s * 512 + q_lane < Lr) {
                        u32 v = row[s * WAVE + lane];
                        const int n_in = Lr - (s * 512 + q_lane);
                        if (n_in < 8) v |= 0xFFFFFFFFu << (4 * n_in);
                        other = other || (((v - 0x11111111u) & ~v & 0x88888888u) != 0u);
                    }
                }
                other_row = __builtin_amdgcn_ballot_w64(other) != 0;
            }
            if (other_row) {
                solo_mask |= 1u << it;
            } else {
                // ---- phase C: stream (recon_lean_kernel's) ----
                PIPE_STAMP_N(k_glob, 7);
                __builtin_amdgcn_s_setprio(0);
                const i64 row0 = cur.base;
                u8 *const oh_row = OH ? cur.onehot + row0 * 4 : nullptr;
                u8 *const hap_row = HAPS ? cur.haps + row0 : nullptr;
                const u32 sel = rc ? 0x0c0c0001u : 0x0c0c0100u;                      // v_perm: 16 bits, byte-swapped for RC
                const u32 tbase = rc ? 256u : 0u;
                const unsigned short *row16 = reinterpret_cast<const unsigned short *>(row);
                if constexpr (RAG) {
                    // Rows of any length that start at any base.  A row's one-hot starts 4 row0 bytes into the output: stored in groups
                    // counted from the ROW's first base, every store instruction's KB begins 4 (row0 & 15) bytes off a 64-byte
                    // boundary, and that costs a quarter of the kernel (tools/ragged_align.py: rows of 2052 bases at k * 2052 take 195 ns
                    // per MB of one-hot, rows of 2064 -- 64 bytes off -- 157, rows of 2048 153).  So the groups are counted from the first
                    // 128-byte boundary of the OUTPUT (RAG_HEAD bases): hh = the bases in front of it (0-31) go out one dword per lane, then body groups
                    // of four at output positions hh + 4 t, t = 64 u + lane -- their 16 nibbles sit at any nibble of the row in LDS
                    // (two 16-bit reads and a shift; reverse-complemented rows read them mirrored: group t holds bases Lr - 4 - hh -
                    // 4 t ..) --, then the last 0-3 bases, again a dword per lane.  (The store instructions issued are COUNTED, see
                    // n_after: the conditions around the body's stores are wave-uniform.)
                    const int hh0 = (OH || ANN) ? (int)((RAG_HEAD - (int)(row0 & (RAG_HEAD - 1))) & (RAG_HEAD - 1)) : 0;
                    const int hh = hh0 < Lr ? hh0 : Lr;
                    const int nb = (Lr - hh) >> 2, tail = (Lr - hh) & 3;
                    const int s0 = rc ? Lr - 4 - hh : hh;                       // the first body group's first base (rc: may be < 0 when nb == 0)
                    const u32 sh = 4u * ((u32)s0 & 3u);
                    const int i0 = s0 >> 2;
                    if (!(ka->dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
#pragma unroll
                        for (int u = 0; u < CFG::MAXT; ++u) {
                            if (u * WAVE < nb) {
                                const int t = u * WAVE + lane;
                                int idx = rc ? i0 - t : i0 + t;
                                idx = idx < 0 ? 0 : idx;
                                const u32 lo16 = row16[idx], hi16 = row16[idx + 1];
                                const u32 r = (((hi16 << 16) | lo16) >> sh) & 0xFFFFu;
                                const u32 rr = __builtin_amdgcn_perm(0u, r, sel);
                                if (t < nb) {
                                    if (OH) {
                                        const uint2 a = lut[tbase + (rr & 0xFFu)], b = lut[tbase + (rr >> 8)];
                                        u32x4_a4 o = {a.x, a.y, b.x, b.y};
                                        store_oh16(oh_row + 4 * (i64)(hh + 4 * t), o);
                                    }
                                    if (HAPS) {
                                        const u32 hb = (u32)blut[tbase + (rr & 0xFFu)] | ((u32)blut[tbase + (rr >> 8)] << 16);
                                        store_u32_unaligned(hap_row + (hh + 4 * t), hb);
                                    }
                                }
                                n_after += (OH ? 1 : 0) + (HAPS ? 1 : 0);
                            }
                        }
                        // head (output positions 0 .. hh - 1: lanes 0 .. RAG_HEAD - 1) and tail (the last `tail` positions: the three lanes behind), a base each
                        // (NOT counted in n_after: the count may fall short of the stores issued -- a stricter wait -- but never exceed them)
                        if (hh > 0 || tail > 0) {
                            const int p = lane < RAG_HEAD ? lane : hh + 4 * nb + (lane - RAG_HEAD);
                            const bool mine = lane < RAG_HEAD ? lane < hh : lane - RAG_HEAD < tail;
                            if (mine) {
                                const int j = rc ? Lr - 1 - p : p;                    // the base that lands at output position p
                                const u32 n4 = (row[j >> 3] >> (4u * ((u32)j & 7u))) & 0xFu;
                                const u32 key = rc ? (256u + (n4 << 4)) : n4;         // (a pair whose other nibble is 0; rc: the table complements the HIGH nibble into its first slot)
                                // (a plain store, not a nontemporal one: the head shares its 128-byte segment with the tail of the row in front, which
                                // another wave of -- three times out of four -- the same workgroup writes: the halves then meet in the L2.  Rows 16 bytes
                                // off a boundary: 191 -> 174 ns per MB of one-hot; the same for the row's last body instruction cost 18 % on every row)
                                if (OH) *reinterpret_cast<u32 *>(oh_row + 4 * (i64)p) = lut[key].x;
                                if (HAPS) hap_row[p] = (u8)blut[key];
                            }
                        }
                    }
                } else if constexpr (CL) {
                    // channel-major planes: a lane takes 16 bases per step (two dwords of the nibble row), 1024 bases per wave-step;
                    // plane c of the row at oh_row + c * L; a reverse-complemented row's bases land mirrored, its channels swapped (the
                    // table's second half) and a lane's four dwords in reverse order
                    if (!(ka->dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
                        n_after += stream_onehot_cl<CFG::MAXT * TRIP>(row, lut, tbase, rc, L, (i64)L, oh_row, lane);
                        if (HAPS) {
                            const i64 hp_lane = rc ? ((i64)L - 4 - 4 * (i64)lane) : 4 * (i64)lane;
                            const int hp_step = rc ? -TRIP : TRIP;
                            const u32 sel_h = rc ? 0x0c0c0001u : 0x0c0c0100u;
#pragma unroll
                            for (int u = 0; u < LEAN_MAX_TRIPS; ++u) {
                                if (u * TRIP < L) {
                                    const u32 rr = __builtin_amdgcn_perm(0u, (u32)row16[u * WAVE + lane], sel_h);
                                    const u32 hb = (u32)blut[tbase + (rr & 0xFFu)] | ((u32)blut[tbase + (rr >> 8)] << 16);
                                    if (u * TRIP + 4 * lane < L) store_u32_unaligned(hap_row + hp_lane + (i64)u * hp_step, hb);
                                    n_after += 1;
                                }
                            }
                        }
                    }
                } else {
                const i64 hp_lane = rc ? ((i64)L - 4 - 4 * (i64)lane) : 4 * (i64)lane;
                const i64 st_lane = 4 * hp_lane;
                const int hp_step = rc ? -TRIP : TRIP;
                const int st_step = 4 * hp_step;
                const u32 lane4 = (u32)lane * GROUP;
                auto stream4 = [&](const int u0) {
                    u32 r[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) r[i] = row16[(u0 + i) * WAVE + lane];
                    uint2 a[4], b[4];
                    u32 hb[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const u32 rr = __builtin_amdgcn_perm(0u, r[i], sel);
                        if (OH) {
                            a[i] = lut[tbase + (rr & 0xFFu)];
                            b[i] = lut[tbase + (rr >> 8)];
                        }
                        if (HAPS) hb[i] = (u32)blut[tbase + (rr & 0xFFu)] | ((u32)blut[tbase + (rr >> 8)] << 16);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (OH) {
                            u32x4_a4 o = {a[i].x, a[i].y, b[i].x, b[i].y};
                            store_oh16(oh_row + st_lane + (i64)(u0 + i) * st_step, o);
                        }
                        if (HAPS) store_u32_unaligned(hap_row + hp_lane + (i64)(u0 + i) * hp_step, hb[i]);
                    }
                };
                if (!(ka->dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
                    if ((L & (4 * TRIP - 1)) == 0) {
                        stream4(0);
                        if (L > 4 * TRIP) stream4(4);
                    } else {
#pragma unroll
                        for (int u = 0; u < LEAN_MAX_TRIPS; ++u) {
                            if (u * TRIP < L) {
                                const u32 r = row16[u * WAVE + lane];
                                const u32 rr = __builtin_amdgcn_perm(0u, r, sel);
                                if (u * TRIP + (int)lane4 < L) {
                                    if (OH) {
                                        const uint2 a = lut[tbase + (rr & 0xFFu)], b = lut[tbase + (rr >> 8)];
                                        u32x4_a4 o = {a.x, a.y, b.x, b.y};
                                        store_oh16(oh_row + st_lane + (i64)u * st_step, o);
                                    }
                                    if (HAPS) {
                                        const u32 hb = (u32)blut[tbase + (rr & 0xFFu)] | ((u32)blut[tbase + (rr >> 8)] << 16);
                                        store_u32_unaligned(hap_row + hp_lane + (i64)u * hp_step, hb);
                                    }
                                }
                            }
                        }
                    }
                    n_after = ((L + TRIP - 1) / TRIP) * ((OH ? 1 : 0) + (HAPS ? 1 : 0));     // store instructions issued
                }
                }
                if constexpr (ANN) {
                    // ---- annotations: per output base {variant index or -1, reference coordinate}.  Forward position p of the row (before a
                    // reverse-complemented row is mirrored) lies in the allele of applied record j iff a_out_j <= p < a_out_j + w_j -- then
                    // {id_j, pos_j} -- else in the reference run behind the last applied indel at or in front of it: {-1, p + delta - contig
                    // start}.  Stored like the ragged one-hot: groups of four counted from the output's first 64-byte boundary (fixed-length
                    // rows: from the row's start, which is one), head / tail positions one per lane; a reverse-complemented row's
                    // annotations are reversed (src/reverse.rs:25-38 on the i32 rows).
                    if (!(ka->dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
                        int *const av_row = cur.av + row0, *const ap_row = cur.ap + row0;
                        const int hh0a = RAG ? (int)((RAG_HEAD - (int)(row0 & (RAG_HEAD - 1))) & (RAG_HEAD - 1)) : 0;
                        const int hha = hh0a < Lr ? hh0a : Lr;
                        const int nba = (Lr - hha) >> 2, taila = (Lr - hha) & 3;
                        const u64 m_app = __builtin_amdgcn_ballot_w64(applied && w_i > 0);
                        // one forward position: every applied record, in order (head / tail lanes; a few positions per row)
                        auto annot1 = [&](const int p, int &id, int &rp) {
                            u32 D = d_init; id = -1; int ps = 0;
                            for (u64 m = m_app; m; m &= m - 1) {
                                const int j = __builtin_ctzll(m);
                                const int a = rdl(a_out, j), w = rdl(w_i, j);
                                if (((m_ns >> j) & 1ull) && p >= a) D = (u32)rdl((int)dv, j);
                                if (p >= a && p < a + w) { id = rdl(vid, j); ps = rdl(pos, j); }
                            }
                            rp = id >= 0 ? ps : (int)((u32)p + D - cs32);
                        };
#pragma unroll 1
                        for (int u = 0; u * WAVE < nba; ++u) {
                            const int t = u * WAVE + lane;
                            const int q0 = hha + 4 * t;                               // the lane's output positions q0 .. q0 + 3
                            const int p0 = rc ? Lr - 4 - q0 : q0;                     // ... hold forward positions p0 .. p0 + 3 (rc: in reverse)
                            const int ts = rc ? Lr - hha - TRIP * (u + 1) : hha + TRIP * u, te = ts + TRIP;      // the trip's forward range
                            // the run the trip begins in, and the records that reach into the trip (scalar: the record lanes' values by readlane)
                            u32 Dbase = d_init;
                            u64 touch = 0;
                            for (u64 m = m_app; m; m &= m - 1) {
                                const int j = __builtin_ctzll(m);
                                const int a = rdl(a_out, j);
                                if (a >= te) break;                                  // (sorted: the rest start behind the trip)
                                const bool nsj = ((m_ns >> j) & 1ull) != 0;
                                if (nsj && a <= ts) Dbase = (u32)rdl((int)dv, j);
                                if (a + rdl(w_i, j) > ts || (nsj && a > ts)) touch |= 1ull << j;
                            }
                            u32 D[4] = {Dbase, Dbase, Dbase, Dbase};
                            int id[4] = {-1, -1, -1, -1}, ps[4] = {0, 0, 0, 0};
                            for (u64 m = touch; m; m &= m - 1) {
                                const int j = __builtin_ctzll(m);
                                const int a = rdl(a_out, j), w = rdl(w_i, j), idj = rdl(vid, j), pj = rdl(pos, j);
                                const u32 dj = (u32)rdl((int)dv, j);
                                const bool nsj = ((m_ns >> j) & 1ull) != 0;
#pragma unroll
                                for (int g = 0; g < 4; ++g) {
                                    const int pg = p0 + g;
                                    if (nsj && pg >= a) D[g] = dj;
                                    if (pg >= a && pg < a + w) { id[g] = idj; ps[g] = pj; }
                                }
                            }
                            int rp[4];
#pragma unroll
                            for (int g = 0; g < 4; ++g) rp[g] = id[g] >= 0 ? ps[g] : (int)((u32)(p0 + g) + D[g] - cs32);
                            if (t < nba) {
                                if (!rc) { store_i32x4(av_row + q0, id[0], id[1], id[2], id[3]); store_i32x4(ap_row + q0, rp[0], rp[1], rp[2], rp[3]); }
                                else { store_i32x4(av_row + q0, id[3], id[2], id[1], id[0]); store_i32x4(ap_row + q0, rp[3], rp[2], rp[1], rp[0]); }
                            }
                            n_after += 2;
                        }
                        if (hha > 0 || taila > 0) {          // (not counted in n_after: see the ragged stream)
                            const int q = lane < RAG_HEAD ? lane : hha + 4 * nba + (lane - RAG_HEAD);
                            const bool mine = lane < RAG_HEAD ? lane < hha : lane - RAG_HEAD < taila;
                            int id1 = -1, rp1 = 0;
                            annot1(rc ? Lr - 1 - q : q, id1, rp1);
                            if (mine) { av_row[q] = id1; ap_row[q] = rp1; }
                        }
                    }
                }
                __builtin_amdgcn_s_setprio(3);
            }
        }
        PIPE_STAMP_N(k_glob, 8);
        if (!more) break;
        // the next row's window + slot line and the entries behind it were requested in FRONT of this row's stores:
        // wait for everything but those stores (rows that stored nothing: for everything)
        wave_lds_fence();                                 // (this row's LDS reads are done before the row after next's DMA may land here)
        wait_vm_all_but(n_after);
        PIPE_STAMP(k_glob, 9);
    }
    if (solo_mask)
        lean_solo_rows<OH, HAPS, CL, ANN>((u64)__builtin_amdgcn_kernarg_segment_ptr(), w_raw, n_waves, solo_mask,
                                 (LutsLds)&solo_luts, (PipeWaveLds)(void *)&pw);
}
