// gvl_lean.inc -- the LEAN reconstruct kernel (included by gvl_hip.hip inside its anonymous namespace).
//
// The all-purpose kernel (recon_body) can express every row the reference's walk can produce
// (src/reconstruct/mod.rs:39-256) and pays for it: ~1200 instructions per row, 153 spilled SGPRs,
// a workgroup-wide head (P1, barriers, packed plan).  The benchmark's rows -- and a real dataset's --
// are almost all of ONE shape: a window that lies inside its contig, at most GVL_SLOT_RECS variants,
// no two of them overlapping.  This kernel streams exactly those rows and nothing else:
//
//   * one wave = one row, no cooperation between the waves of a workgroup beyond the LDS tables:
//     the row's request entries and contig bounds are SCALAR loads (they are wave-uniform), its slot
//     line (gvl_srec, 8 x 16 B) one vector load by lanes 0..7;
//   * reference bases come from the nibble-packed reference (gvl_static.ref4, 4 bits per base:
//     half the bytes / cache lines / DRAM pages of the byte reference behind the cold window
//     reads): per trip of 256 bases one dword per lane = its 4 bases + 4 of slack for odd starts;
//   * the 16 bits of a group go through two 8-byte LDS lookups (nibble pair -> two one-hot dwords);
//     reverse-complement is a second table + a byte swap of the 16 bits + the mirrored store address;
//   * SNPs patch their nibble in registers on their way (sorted, scalar cursor);
//   * rows with indels (src/reconstruct/mod.rs:115-198) keep the same stream: the walk is planned on
//     the row's 8 record lanes (prefix-max check for "first ALT wins", prefix sum for the indel
//     shift) into at most 8 entries {allele start, allele end, reference delta behind it}; a trip
//     inside one reference run only changes its base address, a trip that holds an allele or a run
//     boundary assembles its nibbles per base.
//
// Every row it cannot express exactly -- lead / trail padding, a slot that overflows its line,
// overlapping variants, duplicate positions, a shift that meets an indel, coordinates >= 2^30 -- is
// run by the SAME wave through the all-purpose body in its SOLO mode (recon_body<..., SOLO>: per-wave
// scans or the scalar walk, records from the CSR, bytes from the byte reference).  Bit-exactness is
// therefore never this kernel's judgement call: it either writes the reference's bytes itself or lets
// the walk that is pinned against the reference's goldens write them.
// (Measured and dropped first: listing those rows for a second launch of the all-purpose kernel.  A
// workgroup of that kernel lives ~11 us whatever the number of rows, and the launch waits for the lean
// one: cfg2 26.5 us per batch alone / 12.3 in flight against 13.3 / 8.9 without the lean kernel.)

// what the lean path itself reads: the kernel's FIRST parameter, small enough to be fetched in one go at the
// top (the all-purpose ReconArgs follows it in the kernarg segment; only lean_solo_row looks at that)


// A row the lean path does not take: this wave runs it through the all-purpose body (SOLO).  A real call
// (noinline): the all-purpose body is 5000 instructions with 150 spilled SGPRs, inlined it drags its
// spill code, argument loads and wait counts into the lean path.  The callee finds the launch arguments
// in the kernarg segment (`kernarg` = its address: ReconArgs is the kernel's second parameter, right behind
// LeanArgs; __builtin_amdgcn_kernarg_segment_ptr() is only defined inside the kernel itself).  Its LDS -- the byte tables
// and one SoloLds per wave -- is declared by the KERNEL and handed over as LDS addresses: as function-local __shared__
// arrays of a function that two kernels call (recon_lean_kernel<OH, HAPS, false / true>) they were placed through the
// compiler's per-kernel offset table, and for the <false, true> pair that table put the byte tables at the very end
// of the kernel's LDS allocation (offset == group_segment_fixed_size): every SOLO row came out as pad bytes.
typedef const ReconArgs __attribute__((address_space(4))) *ReconArgsK;
typedef Luts __attribute__((address_space(3))) *LutsLds;
typedef SoloLds<false> __attribute__((address_space(3))) *SoloLdsLds;
template <bool OH, bool HAPS, bool CL = false, bool ANN = false>
__device__ __noinline__ __attribute__((noreturn)) void lean_solo_row(
        const u64 kernarg, const int k, const i64 c_s, const i64 c_e, const int l_start, const int l_shift, const i64 l_oidx, const int rc_shape, const u32 chunk_span,
        const LutsLds luts_lds, const SoloLdsLds solo_lds) {      // chunk_span: first chunk | last chunk << 16 (the wave's chunks still to do)
    Luts &luts = *(Luts *)luts_lds;             // byte tables (filled by the waves that come here: same values from every writer)
    SoloLds<ANN> *const solo_all = (SoloLds<ANN> *)(void *)solo_lds;      // (the kernel's array: SoloLds<ANN> per wave)
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass of the compiler parses this body too and has no address spaces)
    const ReconArgs A = *(ReconArgsK)(u64)(rfl64((i64)kernarg) + (i64)sizeof(LeanArgs));
#else
    const ReconArgs A = ReconArgs();
#endif
    const int lane = threadIdx.x & (WAVE - 1);
    SoloLds<ANN> &solo = solo_all[rfl((int)threadIdx.x >> 6)];
    for (int b = lane; b < 256; b += WAVE) {
        const u32 d = onehot_dword((u32)b);
        luts.oh[b] = d;
        luts.oh_rc[b] = __builtin_bswap32(d);
        luts.comp[b] = (u8)comp_byte((u32)b);
    }
    const i64 oidx = rfl64(l_oidx);
    i64 o_s = 0; int n_var = 0;
    if (rfl(rc_shape) & 2) {
        o_s = A.go_starts[oidx];
        const i64 nv = A.go_stops[oidx] - o_s;
        n_var = nv < 0 ? 0 : (nv > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)nv);
        if (A.dbg & GVL_ABL(DBG_ABL_NO_VARIANTS)) n_var = 0;
    }
    if (lane == 0) {
        RowIn ri;
        const int shift = rfl(l_shift);
        ri.c_s = rfl64(c_s); ri.R = rfl64(c_e) - ri.c_s; ri.ref_start = rfl(l_start); ri.shift = shift;
        ri.o_s = o_s; ri.keep_off = (A.keep && A.keep_offsets) ? A.keep_offsets[rfl(k)] : 0; ri.row_base = (i64)rfl(k) * A.fixed_len;
        ri.k = rfl(k); ri.n_var = n_var; ri.L = (int)A.fixed_len; ri.rc = rfl(rc_shape) & 1;
        ri.flags = (shift < 0 || shift >= (1 << 30)) ? 2 : 0;
        solo.ri = ri;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const u32 span = (u32)rfl((int)chunk_span);
#pragma unroll 1
    for (int c = (int)(span & 0xFFFFu); c <= (int)(span >> 16); ++c) {
        recon_body<OH ? (CL ? OH_CL : OH_LC) : OH_NONE, HAPS, ANN, true>(A, nullptr, &solo, luts, 0, c);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __builtin_amdgcn_endpgm();      // the wave ends here: nothing of the caller has to survive the call
}

// (the same for a row whose place and length the caller names: recon_lean_kernel<.., LONG, RAGL>'s ragged rows)
template <bool OH, bool HAPS>
__device__ __noinline__ __attribute__((noreturn)) void lean_solo_row_at(
        const u64 kernarg, const int k, const i64 c_s, const i64 c_e, const int l_start, const int l_shift, const i64 l_oidx, const int rc_shape, const u32 chunk_span,
        const LutsLds luts_lds, const SoloLdsLds solo_lds, const i64 row_base, const int row_len) {      // chunk_span: first chunk | last chunk << 16 (the wave's chunks still to do)
    Luts &luts = *(Luts *)luts_lds;             // byte tables (filled by the waves that come here: same values from every writer)
    SoloLds<false> *const solo_all = (SoloLds<false> *)solo_lds;
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass of the compiler parses this body too and has no address spaces)
    const ReconArgs A = *(ReconArgsK)(u64)(rfl64((i64)kernarg) + (i64)sizeof(LeanArgs));
#else
    const ReconArgs A = ReconArgs();
#endif
    const int lane = threadIdx.x & (WAVE - 1);
    SoloLds<false> &solo = solo_all[rfl((int)threadIdx.x >> 6)];
    for (int b = lane; b < 256; b += WAVE) {
        const u32 d = onehot_dword((u32)b);
        luts.oh[b] = d;
        luts.oh_rc[b] = __builtin_bswap32(d);
        luts.comp[b] = (u8)comp_byte((u32)b);
    }
    const i64 oidx = rfl64(l_oidx);
    i64 o_s = 0; int n_var = 0;
    if (rfl(rc_shape) & 2) {
        o_s = A.go_starts[oidx];
        const i64 nv = A.go_stops[oidx] - o_s;
        n_var = nv < 0 ? 0 : (nv > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)nv);
        if (A.dbg & GVL_ABL(DBG_ABL_NO_VARIANTS)) n_var = 0;
    }
    if (lane == 0) {
        RowIn ri;
        const int shift = rfl(l_shift);
        ri.c_s = rfl64(c_s); ri.R = rfl64(c_e) - ri.c_s; ri.ref_start = rfl(l_start); ri.shift = shift;
        ri.o_s = o_s; ri.keep_off = (A.keep && A.keep_offsets && !A.ref_only) ? A.keep_offsets[rfl(k)] : 0; ri.row_base = rfl64(row_base);
        ri.k = rfl(k); ri.n_var = n_var; ri.L = rfl(row_len); ri.rc = rfl(rc_shape) & 1;
        ri.flags = (shift < 0 || shift >= (1 << 30)) ? 2 : 0;
        if (A.ref_only) {            // gvl_get_reference's rows: `l_shift` carries the region's END (src/reference/mod.rs:16-18: start >= stop leaves the row as it is)
            ri.shift = 0;
            ri.flags = rfl(l_start) >= shift ? 4 : 0;
        }
        solo.ri = ri;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const u32 span = (u32)rfl((int)chunk_span);
#pragma unroll 1
    for (int c = (int)(span & 0xFFFFu); c <= (int)(span >> 16); ++c) {
        recon_body<OH ? OH_LC : OH_NONE, HAPS, false, true>(A, nullptr, &solo, luts, 0, c);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __builtin_amdgcn_endpgm();      // the wave ends here: nothing of the caller has to survive the call
}

constexpr int LEAN_ROW_DWORDS = LEAN_MAX_TRIPS * TRIP / 8;     // a row of nibbles: 8 bases per dword
constexpr int LEAN_STEPS = LEAN_ROW_DWORDS / WAVE;               // gather steps: 8 bases per lane per step
constexpr int LEAN_TAIL = 64;                                     // bases read speculatively behind the row's own length
constexpr int LEAN_ENT = 32;                                      // LONG: variants that touch one chunk (8 fields each, parked in the row buffer)
static_assert(8 * LEAN_ENT <= LEAN_ROW_DWORDS, "the entries live in the row buffer");

// exclusive prefix scan over the record lanes: lanes 0..7 only (the slot line), or the whole wave
template <typename Op>
__device__ __forceinline__ int lean_scan_excl(const int v, const int lane, const bool short_scans) {
    return short_scans ? seg8_scan_exclusive<Op>(v, lane & 7) : wave_scan_exclusive<Op>(v);
}
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// set nibble `at` (a base position of the row) of the nibble row in LDS; concurrent lanes may hit the same dword
__device__ __forceinline__ void row_set_nibble(u32 *row, const int at, const u32 nib) {
    const u32 sh = 4u * ((u32)at & 7u);
    u32 *w = row + (at >> 3);
    __hip_atomic_fetch_and(w, ~(0xFu << sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __hip_atomic_fetch_or(w, nib << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// ---- channel-major one-hot, (rows, 4, L): what the reference's docs feed a model (docs/source/index.md:114-115 rearranges seqpro's
// (.., L, 4)).  Table: nibble pair b = lo | hi << 4 -> {flags of (lo's base, hi's base) for channel 0 | channel 1 << 16, channel 2 |
// channel 3 << 16}; [256, 512): reverse-complement: the pair's bases in reverse order, channel c = the complement's 3 - c.
// (lo / hi = the nibbles' one-hot dwords: byte c of one is the base's flag for channel c.)
__device__ __forceinline__ void fill_cl_lut(uint2 *lut, const int b, const u32 lo, const u32 hi) {
    auto pairs = [](const u32 a, const u32 b_, const int c) -> u32 { return ((a >> (8 * c)) & 0xFFu) | (((b_ >> (8 * c)) & 0xFFu) << 8); };
    lut[b] = make_uint2(pairs(lo, hi, 0) | (pairs(lo, hi, 1) << 16), pairs(lo, hi, 2) | (pairs(lo, hi, 3) << 16));
    lut[256 + b] = make_uint2(pairs(hi, lo, 3) | (pairs(hi, lo, 2) << 16), pairs(hi, lo, 1) | (pairs(hi, lo, 0) << 16));
}
// Lc bases (a row, or a 2048-base chunk of one; a multiple of 4, at most MAXB) from the nibble row in LDS to the four channel planes:
// plane c's bytes of these bases begin at base + c * plane_stride.  A lane takes 16 bases per step (two dwords of the nibble row),
// 1024 bases per wave-step: a pair of nibbles looks up both bases' flags for all four channels (8 bytes), two v_perm per channel put
// four bases' flags into a dword, and every store instruction writes one contiguous KB of one plane.  A reverse-complemented row's
// bases land mirrored, its channels swapped (the table's second half), a lane's four dwords in reverse order.  -> the FULL store
// instructions issued (the pipelined kernel counts them; the dword stores of a last partial group are not counted: the count may
// fall short of what is issued, never exceed it).
template <int MAXB>
__device__ __forceinline__ int stream_onehot_cl(const u32 *const row32, const uint2 *const lut, const u32 tbase, const bool rc, const int Lc,
                                                const i64 plane_stride, u8 *const base, const int lane) {
    int n_full = 0;
#pragma unroll
    for (int h = 0; h < (MAXB + 1023) / 1024; ++h) {
        if (h * 1024 < Lc) {
            const int q = h * 1024 + 16 * lane;                      // the lane's first base
            const uint2 nb = *reinterpret_cast<const uint2 *>(row32 + (q >> 3));
            uint2 P[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const u32 by = ((i < 4 ? nb.x : nb.y) >> (8 * (i & 3))) & 0xFFu;
                P[i] = lut[tbase + by];
            }
            const int qo = rc ? Lc - 16 - q : q;                     // where the lane's 16 output bytes begin in a plane
            // two channel planes at a time (the table entries' .x, then their .y): 8 dwords in flight, not 16
#pragma unroll
            for (int cp = 0; cp < 2; ++cp) {
                u32 o[2][4];                                         // [channel of the pair][dword of the lane's 16 bytes, in OUTPUT order]
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const u32 pa = cp == 0 ? P[2 * m].x : P[2 * m].y, pb = cp == 0 ? P[2 * m + 1].x : P[2 * m + 1].y;
                    if (!rc) {
                        o[0][m] = __builtin_amdgcn_perm(pb, pa, 0x05040100u); o[1][m] = __builtin_amdgcn_perm(pb, pa, 0x07060302u);
                    } else {
                        o[0][3 - m] = __builtin_amdgcn_perm(pa, pb, 0x05040100u); o[1][3 - m] = __builtin_amdgcn_perm(pa, pb, 0x07060302u);
                    }
                }
                if (q + 16 <= Lc) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        u32x4_a4 v = {o[c][0], o[c][1], o[c][2], o[c][3]};
                        store_oh16(base + (i64)(2 * cp + c) * plane_stride + qo, v);
                    }
                } else if (q < Lc) {
                    // the last 4 / 8 / 12 bases (Lc is a multiple of 4): dword by dword; a reverse-complemented lane's valid dwords are its
                    // LAST ones (output dword d holds bases q + 12 - 4 d ..)
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int bq = rc ? q + 12 - 4 * d : q + 4 * d;   // first base of output dword d
                        if (bq + 4 <= Lc) {
#pragma unroll
                            for (int c = 0; c < 2; ++c)
                                __builtin_nontemporal_store(o[c][d], reinterpret_cast<u32 *>(base + (i64)(2 * cp + c) * plane_stride + (rc ? Lc - 4 - bq : bq)));
                        }
                    }
                }
            }
            if (h * 1024 + 16 <= Lc) n_full += 4;                   // (issued iff lane 0's group is whole)
        }
    }
    return n_full;
}

#ifdef GVL_DIAG
// (s_memtime: the shader clock -- cheap, but only differences inside one wave mean something; stamp 0 also takes
// the 100 MHz real time, slot 10, for the wave's start relative to the launch)
#define LEAN_STAMP(i) do { if (A.stamps && lane == 0) A.stamps[(u64)w_raw * 16 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#define LEAN_NOTE(i, v) do { if (A.stamps && lane == 0) A.stamps[(u64)w_raw * 16 + (i)] = (u64)(v); } while (0)
#else
#define LEAN_STAMP(i) do { } while (0)
#define LEAN_NOTE(i, v) do { } while (0)
#endif

// OH / HAPS: which outputs (one-hot (K, L, 4) and / or haplotype bytes).  Bytes come from the same nibble row through a
// second pair of tables; a nibble that says "some other byte" (IUPAC codes, lower case -- in the reference or in an
// ALT allele) cannot be turned back into its byte, so a bytes-writing row that holds one goes to the SOLO path, which
// reads the byte reference (checked on the finished row, before anything is stored).
//
// LONG: rows longer than one chunk (BASELINE config 4: 131 072 bases).  A wave = one 2048-base chunk of one row, chunks of a
// row are neighbours in the grid.  Such a row has hundreds of variants and its chunk a few: the wave first replays the
// row's walk on the CSR's inline records, 64 variants per trip with carries between the trips (recon_body's P2 + P3
// restated), keeps the walk's state where the chunk begins (the reference delta in front of it) and the variants
// that touch the chunk as <= LEAN_ENT entries in LDS, then reads ITS window at that delta and runs the same phases
// A / B / C on chunk coordinates.  There is no speculative window read (the delta of chunk c depends on every indel
// in front of it) and no slot line.  A chunk it cannot express runs the all-purpose body for that chunk (SOLO).
// RAGL (with LONG): RAGGED long rows -- row k at out_offsets[k] .. out_offsets[k + 1] (output_length = -1, the reference's default
// output, src/ffi/mod.rs:794-815), any length: the grid has the chunks of the caller's bound on the longest row, a row's waves
// beyond its own length end at once, its last chunk may end in a group of 1-3 bases (stored dword by dword / byte by byte, as
// recon_lean_rows_kernel's ragged form does).  A row longer than the bound goes to the all-purpose body, which reports it.
// CL (with LONG, fixed-length rows): channel-major one-hot (rows, 4, Lrow) -- config 4's rows as a model takes them.
// ANN (with LONG, fixed-length rows, round 6): annotated haplotypes at any length (src/ffi/mod.rs:2237-2397) -- bytes + per base the variant
// it comes from (-1: the reference) and its reference coordinate, as recon_lean_rows_kernel's ANN form writes them for rows of one
// chunk.  The walk keeps every entry's variant index and position; chunk plans carry them in an annex behind their entries.
template <bool OH, bool HAPS, bool LONG, bool RAGL = false, bool CL = false, bool ANN = false>
__global__ __launch_bounds__(LEAN_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void recon_lean_kernel(const LeanArgs A, const ReconArgs RA) {
    static_assert(!RAGL || LONG, "ragged rows of at most 2560 bases take recon_lean_rows_kernel");
    static_assert(!CL || (OH && LONG && !RAGL), "channel-major one-hot: fixed-length rows; rows of one chunk take recon_lean_rows_kernel's form");
    static_assert(!ANN || (LONG && HAPS && !RAGL), "annotated long rows: fixed length, bytes + both annotation streams (+ a one-hot in either layout)");
    if constexpr (!LONG) __builtin_amdgcn_s_setprio(3);
    // [0, 256): nibble pair -> {one-hot of the low nibble, one-hot of the high nibble};
    // [256, 512): reverse-complement: {one-hot of the HIGH nibble's complement, of the low nibble's}
    __shared__ uint2 lut[OH ? 512 : 1];
    // the same for bytes: nibble pair -> its two bytes (low nibble first); reverse-complement: complements, high nibble first
    __shared__ unsigned short blut[HAPS ? 512 : 1];
    // the row as nibbles in OUTPUT coordinates: gathered from the packed reference run by run (phase A),
    // patched with SNPs and allele bytes (phase B), streamed out through the tables (phase C)
    __shared__ u32 rows[LEAN_WAVES][LEAN_ROW_DWORDS + LEAN_TAIL / 8 + 2];
    // lean_solo_row's: byte tables + per-wave tables of the all-purpose body (only rows that go SOLO touch them)
    __shared__ Luts solo_luts;
    __shared__ SoloLds<ANN> solo_all[LEAN_WAVES];
    // ANN: the entries' variant indices and positions (the row buffer holds the other eight fields)
    __shared__ u32 ann_ent[ANN ? LEAN_WAVES : 1][ANN ? 2 * LEAN_ENT : 1];

    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = rfl(tid >> 6);
    const int w_raw = (int)blockIdx.x * LEAN_WAVES + wave;
    int k_raw = w_raw, chunk0 = 0, n_sub = 1;        // LONG: the wave takes chunks [chunk0, chunk0 + n_sub) of row k_raw
    if constexpr (LONG) {
        const u32 per_row = ((u32)A.chunks + (u32)A.sub - 1u) / (u32)A.sub;
        k_raw = (int)((u32)w_raw / per_row);
        chunk0 = (w_raw - k_raw * (int)per_row) * A.sub;
        n_sub = A.chunks - chunk0 < A.sub ? A.chunks - chunk0 : A.sub;
    }
    const bool is_row = k_raw < A.n_rows;
    const int k = is_row ? k_raw : 0;
    typename std::conditional<RAGL, int, const int>::type Lrow = A.L;      // the row (L, below: the chunk in hand; lo: where that starts; RAGL: from out_offsets)
    if (is_row) { LEAN_NOTE(10, __builtin_amdgcn_s_memrealtime()); LEAN_STAMP(0); }

    // ---- level 1: the row's request entries.  Wave-uniform, so they are SCALAR loads: read through pointers into the
    // constant address space, which is what makes the compiler pick s_load (for a uniform GLOBAL address it chose
    // s_load or a vector load + readfirstlane + vmcnt(0) differently with every edit of this kernel) and lets it keep
    // track of when they land.  (They were inline-asm s_loads with a separate asm wait once: the compiler may copy or
    // spill an asm output between the two statements -- before the load has landed -- and did, for two of the six
    // instances, as soon as the scalar side got tighter.)
#if defined(__HIP_DEVICE_COMPILE__)
    // (every kernel argument the entries' addresses are made of is fetched FIRST -- named as scalar operands of an empty
    // statement -- or the compiler fetches one of them between two entry loads and waits for the first entry to land
    // before it asks for the others: two memory round trips in a row instead of one)
    asm volatile("" :: "s"(A.regions), "s"(A.regions_stride), "s"(A.shifts), "s"(A.geno_offset_idx), "s"(A.to_rc), "s"(A.ref_offsets),
                 "s"(A.n_contigs), "s"(A.ploidy_shift), "s"(A.ploidy), "s"(A.srec), "s"(A.ref4), "s"(A.n_geno_offsets));
#endif
    const int query = A.ploidy_shift >= 0 ? (k >> A.ploidy_shift) : (int)((u32)k / (u32)A.ploidy);
    const int *p_reg = A.regions + (i64)query * A.regions_stride;
    // (RAGL launches may be gvl_get_reference's -- ref_only: no shifts, no genotypes; the "shift" entry carries the region's END
    // instead, as in recon_lean_rows_kernel)
    const bool ref_only = RAGL && A.ref_only != 0;
    const int *p_shift = ref_only ? p_reg + 2 : A.shifts + k;
    const i64 *p_oidx = ref_only ? reinterpret_cast<const i64 *>(p_reg) : A.geno_offset_idx + k;
    // to_rc is a byte array: read the byte's aligned dword (it never leaves the byte's own page)
    const u8 *pb = A.to_rc ? A.to_rc + k : reinterpret_cast<const u8 *>(A.regions);
    const u32 rc_mis = (u32)(u64)pb & 3u;
    const u8 *p_rc = pb - rc_mis;
    // (with them, lane l asks for contig l's bounds -- a dataset has a few dozen contigs: the row's own are then a readlane
    // away when its contig number arrives, not a dependent load)
    const bool ro_lanes = !LONG && A.n_contigs < WAVE;
    i64 ro_l = 0;
    if (ro_lanes && lane <= A.n_contigs) ro_l = A.ref_offsets[lane];
    typedef const int __attribute__((address_space(4))) *KInt;
    typedef const u32 __attribute__((address_space(4))) *KU32;
    typedef const i64 __attribute__((address_space(4))) *KI64;
    const int l_c = ((KInt)(u64)p_reg)[0], l_start = ((KInt)(u64)p_reg)[1];
    const int l_shift_raw = *(KInt)(u64)p_shift;
    const i64 l_oidx_raw = *(KI64)(u64)p_oidx;
    const int l_shift = ref_only ? 0 : l_shift_raw;
    const int l_end = l_shift_raw;                   // (ref_only: what the entry holds)
    const i64 l_oidx = ref_only ? 0 : l_oidx_raw;
    const u32 l_rcw = *(KU32)(u64)p_rc;
    i64 l_o0 = 0, l_o1 = 0;
    if constexpr (RAGL) { l_o0 = ((KI64)(u64)(A.out_offsets + k))[0]; l_o1 = ((KI64)(u64)(A.out_offsets + k))[1]; }
    // (LONG: a keep mask -- the spliced path's exonic filter, src/genotypes/mod.rs:127-176 -- hides variants from the walk: the row's
    // first keep byte is keep[keep_offsets[k]])
    const bool has_keep = LONG && A.keep != nullptr && A.keep_offsets != nullptr && !ref_only;
    i64 l_ko = 0;
    if (has_keep) l_ko = *(KI64)(u64)(A.keep_offsets + k);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" :: "s"(l_c), "s"(l_start), "s"(l_shift_raw), "s"(l_oidx_raw), "s"(l_rcw));     // (one round: see above)
    if constexpr (RAGL) asm volatile("" :: "s"(l_o0), "s"(l_o1));
#endif
    {   // tables, while the loads are out
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
    if (is_row) LEAN_STAMP(1);
    const bool rc = A.to_rc != nullptr && ((l_rcw >> (8u * rc_mis)) & 0xFFu) != 0;

    // ---- level 2: contig bounds (scalar) and the slot line (lanes 0..7) -------------------------------
    const bool c_ok = (u32)l_c < (u32)A.n_contigs;
    i64 c_s, c_e;
    if (ro_lanes) {
        const int cc = c_ok ? l_c : 0;
        c_s = (i64)(((u64)(u32)rdl((int)(u32)((u64)ro_l >> 32), cc) << 32) | (u32)rdl((int)(u32)(u64)ro_l, cc));
        c_e = (i64)(((u64)(u32)rdl((int)(u32)((u64)ro_l >> 32), cc + 1) << 32) | (u32)rdl((int)(u32)(u64)ro_l, cc + 1));
    } else {
        const i64 *p_ro = A.ref_offsets + (c_ok ? l_c : 0);
        c_s = ((KI64)(u64)p_ro)[0]; c_e = ((KI64)(u64)p_ro)[1];
    }
    const bool o_ok = ref_only || (l_oidx >= 0 && l_oidx < A.n_geno_offsets);
    i32x4 rec = {0, 0, (int)GVL_SREC_EMPTY, 0};
    i64 l_gs = 0, l_ge = 0;                      // LONG: the row's CSR bounds
    if constexpr (LONG) {
        if (!ref_only) {
            l_gs = *(KI64)(u64)(A.go_starts + (o_ok ? l_oidx : 0));
            l_ge = *(KI64)(u64)(A.go_stops + (o_ok ? l_oidx : 0));
        }
    } else {
        if (lane < GVL_SLOT_RECS)
            rec = *reinterpret_cast<const i32x4 *>(A.srec + ((o_ok ? l_oidx : 0) * GVL_SLOT_RECS + lane));
    }
    // one-chunk form: the speculative window reads (see issue_window below) go out HERE, in front of the tables' barrier -- the
    // row's contig bounds are known (readlane), nothing else is needed for the address
    u64 xw_e[LEAN_STEPS], xw_tail_e = 0;
    if constexpr (!LONG) {
        const i64 R64e = c_e - c_s;
        const bool row_e = c_ok && o_ok && l_start >= 0 && l_start < (1 << 30) && l_shift >= 0 && l_shift < (1 << 30) &&
                           R64e >= 0 && R64e < (1ll << 31) && !(A.dbg & DBG_LEAN_SOLO);
        const int r0e = l_start + l_shift;
        const u32 G0e = (u32)c_s + (u32)r0e;
        if (row_e && (i64)r0e + Lrow <= R64e && !(A.dbg & GVL_ABL(DBG_ABL_NO_LOADS))) {
            const u8 *wb = A.ref4 + (G0e >> 1) + 4u * (u32)lane;
#pragma unroll
            for (int s = 0; s < LEAN_STEPS; ++s)
                if (s * 512 < Lrow) __builtin_memcpy(&xw_e[s], wb + s * 256, 8);
            if (lane < LEAN_TAIL / 8) __builtin_memcpy(&xw_tail_e, wb + ((Lrow + 7) >> 3) * 4, 8);
        } else {
#pragma unroll
            for (int s = 0; s < LEAN_STEPS; ++s) xw_e[s] = 0;
        }
    }
    // the tables' barrier sits where the wave waits for its scalar loads anyway; LDS-only (no vmcnt), so the
    // slot line and the window stay in flight across it
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (!is_row) return;
    bool too_long = false;
    if constexpr (RAGL) {
        const i64 len64 = l_o1 - l_o0;
        too_long = len64 > (i64)A.chunks * (LEAN_MAX_TRIPS * TRIP);          // (beyond the launch's grid: the all-purpose body reports it)
        Lrow = len64 < 0 ? 0 : (too_long ? A.chunks * (LEAN_MAX_TRIPS * TRIP) : (int)len64);
        const int my_chunks = (Lrow + LEAN_MAX_TRIPS * TRIP - 1) / (LEAN_MAX_TRIPS * TRIP);
        if (chunk0 >= my_chunks) return;
        n_sub = my_chunks - chunk0 < n_sub ? my_chunks - chunk0 : n_sub;
    }
    LEAN_STAMP(2);
    if (A.out_offsets_w && lane == 0 && chunk0 == 0) {
        A.out_offsets_w[k] = (i64)k * Lrow;
        if (k == A.n_rows - 1) A.out_offsets_w[k + 1] = (i64)(k + 1) * Lrow;
    }

    // LONG: a wave takes A.sub consecutive chunks of its row one after the other, and the walk of a chunk resumes where
    // the chunk before it ended -- at the top of the 64-variant trip in which that one saw its last variant -- instead
    // of at the row's first variant (every chunk-wave for itself replayed 1.4 trips too many on average, a fifth of
    // the kernel's instructions on BASELINE config 4; the row's request entries and tables are read once per wave)
    int rs_tb = 0, rs_rem = 0, rs_ref0 = 0, rs_pm = 0, rs_x = 0, rs_posc = -1, rs_refend = 0, rs_outend = 0;
    bool rs_have = false, rs_any = false;
    u32 rs_dlast = 0;
#pragma unroll 1
    for (int sub = 0; sub < (LONG ? n_sub : 1); ++sub) {
    const int chunk = chunk0 + sub;
    const int lo = LONG ? chunk * (LEAN_MAX_TRIPS * TRIP) : 0;
    const int L = LONG ? ((Lrow - lo < LEAN_MAX_TRIPS * TRIP) ? Lrow - lo : LEAN_MAX_TRIPS * TRIP) : Lrow;
    // ---- the window.  Everything below is i32 / u32: contig coordinates < 2^30, positions of the packed
    // reference < 2^32 (the host checks ref_len) -------------------------------------------------------
    const i64 R64 = c_e - c_s;
    bool lean_row = c_ok && o_ok && l_start >= 0 && l_start < (1 << 30) && l_shift >= 0 && l_shift < (1 << 30) &&
                    R64 >= 0 && R64 < (1ll << 31) && !(A.dbg & DBG_LEAN_SOLO) && !too_long;
    // (padded_slice, src/reference/mod.rs:9-50: start >= stop leaves the row untouched, a stop behind the contig pads: not this path's rows)
    if (ref_only) lean_row = lean_row && l_start < l_end && (i64)l_end <= R64;
    const int R = (int)R64;
    const u32 cs32 = (u32)c_s, ce32 = (u32)c_e;
    const int r0 = l_start + l_shift;            // contig coordinate of output position 0 when nothing but SNPs is in the way
    u32 G0 = cs32 + (u32)r0;                     // ... as a position of the packed reference (LONG: set by the walk)
    bool spec_ok = lean_row && (i64)r0 + L <= R64;           // that reading needs no padding
    const int q_lane = 8 * lane;                 // phase A: lane owns bases [512 s + 8 lane, + 8) of step s

    // speculative window reads (exact for rows without indels): 8 bases + 8 of slack per lane per step.
    // No lane predicate: ref4's padding (GVL_REF4_PAD) covers a whole row from any start inside the reference.
    // Lanes 0..7 read LEAN_TAIL more bases behind the row: what a row with deletions needs beyond its own length.
    // (LONG: the same reads, issued once the walk has told where the chunk's window is.)
    u64 xw[LEAN_STEPS], xw_tail = 0;
    auto issue_window = [&]() {
        if (spec_ok && !(A.dbg & GVL_ABL(DBG_ABL_NO_LOADS))) {
            const u8 *wb = A.ref4 + (G0 >> 1) + 4u * (u32)lane;
#pragma unroll
            for (int s = 0; s < LEAN_STEPS; ++s)
                if (s * 512 < L) __builtin_memcpy(&xw[s], wb + s * 256, 8);
            if (lane < LEAN_TAIL / 8) __builtin_memcpy(&xw_tail, wb + ((L + 7) >> 3) * 4, 8);
        } else {
#pragma unroll
            for (int s = 0; s < LEAN_STEPS; ++s) xw[s] = 0;
        }
    };
    if constexpr (!LONG) {
#pragma unroll
        for (int s = 0; s < LEAN_STEPS; ++s) xw[s] = xw_e[s];
        xw_tail = xw_tail_e;
    }

    // ---- the row's variants: lane j = variant j.  The slot line holds at most 8; a slot that overflows it
    // (GVL_SREC_OVERFLOW) reads up to 64 from the CSR's inline records -- three more dependent reads, rare.
    // (LONG: lane j = entry j, the variants of the row that touch this chunk.)
    int n_rec = GVL_SLOT_RECS;
    bool short_scans = true;                     // (prefix scans over 8 record lanes: 3 DPP steps instead of 7)
    bool valid = false, is_snp = false;
    int alen = 0, alen0 = 0, altoff = 0;         // allele bytes in the row (a shift may cut its front off) / in the allele; where they are
    u32 inl = 0;                                 // the allele's first byte
    int why = lean_row ? 0 : 1;                  // (diagnostic builds: why a row went solo)
    u64 m_ins = 0;
    // ---- allele bytes behind an allele's first byte (insertions) live in alt_alleles.  Which of them the row uses
    // is the plan's business, WHERE they are is known now: number them through (lane t = byte t of the row's
    // alleles, pb_first = a variant's first number) and request the first 64 before the plan, so that the read
    // is back when phase B wants it -- an insertion then costs no memory round trip of its own.
    int pb_first = 0, pb_total = 0;
    int pb_owner = 0, pb_i = 0; u32 pb_v = 0;    // lane t: byte pb_i of variant pb_owner's allele
    auto allele_byte_of = [&](const int t, int &owner, int &i) -> const u8 * {
        owner = 0;
        for (u64 m = m_ins; m; m &= m - 1) {
            const int j = __builtin_ctzll(m);
            if (t >= rdl(pb_first, j)) owner = j;
        }
        i = t - bperm(owner, pb_first) + 1;
        return A.alt_alleles + ((u32)bperm(owner, altoff) + (u32)i);
    };
    auto issue_allele_bytes = [&]() {
        if (m_ins) {
            pb_first = lean_scan_excl<OpSat>((valid && alen0 > 1) ? alen0 - 1 : 0, lane, short_scans);
            const int last = 63 - __builtin_clzll(m_ins);
            pb_total = OpSat::f(rdl(pb_first, last), rdl(alen0, last) - 1);
            const u8 *src = allele_byte_of(lane < pb_total ? lane : 0, pb_owner, pb_i);      // (every lane: it shuffles between lanes)
            if (lane < pb_total && !(A.dbg & GVL_ABL(DBG_ABL_NO_LOADS))) pb_v = (u32)*src;
        }
    };
    // ---- plan: which variants are applied, where their alleles start in the row (the indel shift), and the
    // reference position behind each indel.  src/reconstruct/mod.rs:85-198 restated as in recon_body's P3.
    bool applied = false, nonsnp = false;
    int skip_l = 0;                              // bytes a shift cut off the front of this lane's allele (:131-146)
    int a_out = 0, w_i = 0;                      // allele start / bytes written (output coordinates)
    u32 dv = 0;                                  // packed-reference position minus output position, behind this variant
    u32 d_init = G0;                             // ... and in front of the first applied indel
    int e_vid = -1, e_pos = 0;                   // ANN: the entry's variant index and position

    if constexpr (LONG) {
        // ---- the row's walk, 64 variants per trip, carries between the trips (recon_body's P2 + P3 restated).  Row
        // coordinates.  What the chunk needs of it: d_first = the delta behind the last indel whose allele starts at or
        // in front of the chunk's first base, and the applied variants whose allele bytes fall into [lo, hi) as entries
        // in LDS (struct of arrays in the wave's row buffer, which is free until phase A): allele start relative to the
        // chunk, bytes written, allele length as cut by the shift / as stored, delta behind it (chunk coordinates),
        // first byte + SNP flag, offset of the allele's bytes, bytes cut by the shift.
        // With a plan (hap_plan_kernel, below: the row walked ONCE, per launch or per epoch) the chunk needs none of this: where its
        // window is and its entries are two reads away.
        bool planned = false;
        if (A.hplan != nullptr && lean_row) {
            const u32 *const hp = A.hplan + ((i64)k * A.chunks + chunk) * (i64)HP_STRIDE_DW;
            const u32 h0 = ((KU32)(u64)hp)[0], h1 = ((KU32)(u64)hp)[1];
            if (h1 & 0x100u) {
                planned = true;
                const int n_pe = (int)(h1 & 0xFFu);
                i32x4 e0 = {0, 0, 0, 0}, e1 = {0, 0, 0, 0};
                if (lane < n_pe) {           // (in front of the window reads: they are waited for first)
                    e0 = *reinterpret_cast<const i32x4 *>(hp + 4 + 8 * lane);
                    e1 = *reinterpret_cast<const i32x4 *>(hp + 8 + 8 * lane);
                    if constexpr (ANN) {
                        const int2 ax = *reinterpret_cast<const int2 *>(hp + HP_ANNEX_DW + 2 * lane);
                        e_vid = ax.x; e_pos = ax.y;
                    }
                }
                G0 = h0; d_init = h0;
                spec_ok = (h1 & 0x200u) != 0;
                issue_window();
                n_rec = n_pe;
                short_scans = true;
                valid = lane < n_pe;
                if (valid) {
                    a_out = e0.x; w_i = e0.y; alen = e0.z; alen0 = e0.w;
                    dv = (u32)e1.x;
                    inl = (u32)e1.y & 0xFFu; is_snp = ((u32)e1.y & 256u) != 0;
                    altoff = e1.z; skip_l = e1.w;
                    applied = true;
                    nonsnp = !is_snp;
                }
                m_ins = __builtin_amdgcn_ballot_w64(valid && alen0 > 1);
                issue_allele_bytes();
            }
        }
        if (!planned) {
        const i64 o_s = (i64)l_gs;
        const i64 nv64 = (i64)l_ge - o_s;
        bool ok = lean_row && (ref_only || A.grec != nullptr) && nv64 >= 0 && nv64 < (1ll << 30);
        if (lean_row && !ok) why = 2;
        const int n_var = ok ? (int)nv64 : 0;
        const int hi = lo + L;
        u32 *const ent = rows[wave];
        int rem = l_shift, ref_idx0 = l_start, pm_carry = l_start, x_carry = 0, pos_carry = -1;
        bool ended = false, past = false, have_first = false;
        u32 d_first = 0;
        int ref_idx_end = l_start, out_idx_end = 0;
        int tb0 = 0;
        // resume behind the chunk before (its last trip is run again from the state at its top).  Everything in front
        // of that trip lies in front of this chunk -- unless an allele from there reaches into it (an insertion longer
        // than what was left of the chunk before): then the walk starts over
        if (rs_any && rs_outend <= lo) {
            tb0 = rs_tb; rem = rs_rem; ref_idx0 = rs_ref0; pm_carry = rs_pm; x_carry = rs_x; pos_carry = rs_posc;
            ref_idx_end = rs_refend; out_idx_end = rs_outend; have_first = rs_have; d_first = rs_dlast;
        }
        bool have_last = have_first; u32 d_last = d_first;       // the delta behind the last applied indel so far
        int s_tb = 0, s_rem = 0, s_ref0 = 0, s_pm = 0, s_x = 0, s_posc = -1, s_refend = 0, s_outend = 0;
        bool s_have = false, s_any = false;
        u32 s_dlast = 0;
        int n_ent = 0;
        const i32x4 rec_none = {0, 0, 0, 0};
        i32x4 nxt = rec_none;
        u32 nxt_keep = 1;
        if (tb0 + lane < n_var) {
            nxt = *reinterpret_cast<const i32x4 *>(A.grec + (o_s + tb0 + lane));
            if (has_keep) nxt_keep = (u32)A.keep[l_ko + tb0 + lane];
        }
#pragma unroll 1
        for (int tb = tb0; tb < n_var && ok && !ended && !past; tb += WAVE) {
            s_tb = tb; s_rem = rem; s_ref0 = ref_idx0; s_pm = pm_carry; s_x = x_carry; s_posc = pos_carry;
            s_refend = ref_idx_end; s_outend = out_idx_end; s_have = have_last; s_dlast = d_last; s_any = true;
            const i32x4 r = nxt;
            const bool kept = nxt_keep != 0;
            nxt = rec_none;
            nxt_keep = 1;
            if (tb + WAVE + lane < n_var) {
                nxt = *reinterpret_cast<const i32x4 *>(A.grec + (o_s + tb + WAVE + lane));
                if (has_keep) nxt_keep = (u32)A.keep[l_ko + tb + WAVE + lane];
            }
            const bool in_row = tb + lane < n_var;
            const bool v = in_row && kept;                  // (a masked variant does not exist for the walk: src/reconstruct/mod.rs:86-90)
            const int pos = r.x, d = r.y, vi = r.w;
            int al = (int)((u32)r.z >> 8);
            const int al0 = al;
            const u32 in_ = (u32)r.z & 0xFFu;
            int skip = 0;
            const int pos_prev = dpp_mov<0x138, 0xf>(pos_carry, pos);           // wave_shr:1 (lane 0: the trip before)
            const u64 m_bad = __builtin_amdgcn_ballot_w64(
                in_row && (pos < 0 || pos >= (1 << 30) || d <= -(1 << 30) || d >= (1 << 30) || al >= 0xFFFFFF || pos < pos_prev));
            if (m_bad) { ok = false; why = 3; break; }
            pos_carry = rdl(pos, WAVE - 1);
            const int E = pos - (d < 0 ? d : 0) + 1;                            // v_ref_end, :96
            const bool snp = d == 0 && al == 1;
            // DEL spanning the window start (:99-102): the last one in order sets ref_idx (nothing is applied yet)
            const u64 m_span = __builtin_amdgcn_ballot_w64(v && pos < l_start && d < 0 && E >= l_start);
            if (m_span) { ref_idx0 = rdl(E, 63 - __builtin_clzll(m_span)); pm_carry = ref_idx0; ref_idx_end = ref_idx0; }
            bool cand = v && pos >= l_start;
            if (rem > 0) {      // shift consumption (:115-146)
                const int base = ref_idx0;
                const u64 m_t = __builtin_amdgcn_ballot_w64(cand && pos >= base && (pos - base) + al >= rem);
                if (m_t == 0) {
                    cand = false;                       // still open after this trip
                } else {
                    const int f = __builtin_ctzll(m_t);
                    const int dist = rdl(pos, f) - base;
                    if (dist >= rem) {
                        ref_idx0 = base + rem;
                        cand = cand && lane >= f;
                    } else {
                        const int sk = rem - dist;
                        if (sk == rdl(al, f)) {
                            ref_idx0 = rdl(E, f);
                            cand = cand && lane > f;
                        } else {
                            ref_idx0 = rdl(pos, f);
                            cand = cand && lane >= f;
                            if (lane == f) { al -= sk; skip = sk; }
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
                if (!stable) { ok = false; why = 5; break; }
            }
            const int n_i = inB ? pos - PM : 0;
            const int S_i = inB ? OpSat::f(n_i, al) : 0;
            int x_incl;
            const int X = OpSat::f(x_carry, wave_scan_exclusive<OpSat>(S_i, x_incl));
            const int ao = OpSat::f(X, n_i);                                     // allele start, row coordinates
            const bool app = inB && ao < Lrow;                                   // :154-158 break
            const int wi = app ? ((al < Lrow - ao) ? al : Lrow - ao) : 0;       // :178
            const bool ns = app && !snp;
            const u64 m_inB = __builtin_amdgcn_ballot_w64(inB);
            const u64 m_app = __builtin_amdgcn_ballot_w64(app);
            if (m_inB != m_app) ended = true;
            if (m_app) {
                const int last = 63 - __builtin_clzll(m_app);
                ref_idx_end = rdl(E, last);
                out_idx_end = rdl(ao, last) + rdl(wi, last);
                if (rdl(ao, last) >= hi) past = true;
            }
            const u32 dvr = cs32 + (u32)E - (u32)(ao + al);                     // delta behind this variant, row coordinates
            const u64 m_before = __builtin_amdgcn_ballot_w64(ns && ao <= lo);
            if (m_before) { d_first = (u32)rdl((int)dvr, 63 - __builtin_clzll(m_before)); have_first = true; }
            const u64 m_ns_all = __builtin_amdgcn_ballot_w64(ns);
            if (m_ns_all) { d_last = (u32)rdl((int)dvr, 63 - __builtin_clzll(m_ns_all)); have_last = true; }
            const bool touch = app && ao < hi && ao + wi > lo;
            const u64 m_touch = __builtin_amdgcn_ballot_w64(touch);
            const int n_new = __builtin_popcountll(m_touch);
            if (n_ent + n_new > LEAN_ENT) { ok = false; why = 2; break; }
            if (touch) {
                const int q = n_ent + __builtin_popcountll(m_touch & ((1ull << lane) - 1ull));
                ent[0 * LEAN_ENT + q] = (u32)(ao - lo);
                ent[1 * LEAN_ENT + q] = (u32)wi;
                ent[2 * LEAN_ENT + q] = (u32)al;
                ent[3 * LEAN_ENT + q] = (u32)al0;
                ent[4 * LEAN_ENT + q] = dvr + (u32)lo;
                ent[5 * LEAN_ENT + q] = in_ | (snp ? 256u : 0u);
                // (only an allele with bytes behind its first needs its offset; a SNP's or a deletion's anchor is inline)
                ent[6 * LEAN_ENT + q] = al0 > 1 ? (u32)(u64)A.alt_offsets[vi] : 0u;
                ent[7 * LEAN_ENT + q] = (u32)skip;
                if constexpr (ANN) { ann_ent[wave][q] = (u32)vi; ann_ent[wave][LEAN_ENT + q] = (u32)pos; }
            }
            n_ent += n_new;
            if (tb + WAVE < n_var) {        // carries (pm_incl: the scan of the last fixed-point round = the final mask's)
                const int mx = rdl(pm_incl, WAVE - 1);
                pm_carry = mx > pm_carry ? mx : pm_carry;
                x_carry = OpSat::f(x_carry, rdl(x_incl, WAVE - 1));
            }
        }
        if (ok) {
            if (rem > 0) {                            // the shift never completed: nothing was applied
                const i64 t = (i64)ref_idx0 + rem;
                ref_idx_end = (int)(t < R64 ? t : R64);
            }
            // a walk that ran to its end: the tail (:200-255) must reach the chunk's end without padding
            if (!ended && !past && hi - out_idx_end > 0 && (i64)(hi - out_idx_end) > R64 - (i64)ref_idx_end) { ok = false; why = 6; }
            const u32 d0 = have_first ? d_first : cs32 + (u32)(rem > 0 ? ref_idx_end : ref_idx0);
            G0 = d0 + (u32)lo;                        // where the chunk's first base comes from
            d_init = G0;
            const int rel0 = (int)(G0 - cs32);        // (negative: the chunk begins inside an allele that is longer than the contig in front of it)
            spec_ok = ok && rel0 >= 0 && (i64)rel0 + L <= R64;
        }
        if (ok && s_any) {
            rs_tb = s_tb; rs_rem = s_rem; rs_ref0 = s_ref0; rs_pm = s_pm; rs_x = s_x; rs_posc = s_posc;
            rs_refend = s_refend; rs_outend = s_outend; rs_have = s_have; rs_dlast = s_dlast; rs_any = true;
        }
        lean_row = ok;
        issue_window();
        wave_lds_fence();
        n_rec = n_ent;
        short_scans = n_rec <= 8;
        valid = lean_row && lane < n_ent;
        if (valid) {
            a_out = (int)ent[0 * LEAN_ENT + lane]; w_i = (int)ent[1 * LEAN_ENT + lane];
            alen = (int)ent[2 * LEAN_ENT + lane]; alen0 = (int)ent[3 * LEAN_ENT + lane];
            dv = ent[4 * LEAN_ENT + lane];
            const u32 f = ent[5 * LEAN_ENT + lane];
            inl = f & 0xFFu; is_snp = (f & 256u) != 0;
            altoff = (int)ent[6 * LEAN_ENT + lane]; skip_l = (int)ent[7 * LEAN_ENT + lane];
            if constexpr (ANN) { e_vid = (int)ann_ent[wave][lane]; e_pos = (int)ann_ent[wave][LEAN_ENT + lane]; }
            applied = true;
            nonsnp = !is_snp;
        }
        wave_lds_fence();                            // (phase A reuses the buffer)
        m_ins = __builtin_amdgcn_ballot_w64(valid && alen0 > 1);
        issue_allele_bytes();
        }       // (!planned)
    } else {
        bool ovf_solo = false;
        if (lean_row && rfl(rec.z) == (int)GVL_SREC_OVERFLOW) {
            ovf_solo = true;
            if (A.grec) {
                const i64 o_s = A.go_starts[l_oidx];
                const i64 nv = A.go_stops[l_oidx] - o_s;
                if (nv >= 0 && nv <= WAVE) {
                    ovf_solo = false;
                    n_rec = (int)nv;
                    rec.x = 0; rec.y = 0; rec.z = (int)GVL_SREC_EMPTY; rec.w = 0;
                    if (lane < n_rec) {
                        rec = *reinterpret_cast<const i32x4 *>(A.grec + (o_s + lane));
                        const u32 ee = (u32)rec.z;
                        // (only an allele with bytes behind its first needs its offset; a SNP's or a deletion's anchor is inline)
                        rec.w = (ee >> 8) > 1u ? (int)(u32)(u64)A.alt_offsets[rec.w] : 0;
                    }
                }
            }
        }
        short_scans = n_rec <= 8;
#ifdef GVL_DIAG
        if (A.stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); LEAN_STAMP(3); }      // records AND the speculative window are back
#endif
        const u32 e = (u32)rec.z;
        valid = lane < n_rec && e != GVL_SREC_EMPTY && e != GVL_SREC_OVERFLOW;
        const int pos = rec.x, d = rec.y;
        alen = (int)(e >> 8);
        inl = e & 0xFFu;
        u32 a0 = (u32)rec.w;
        is_snp = d == 0 && alen == 1;
        const int pos_prev = dpp_mov<0x138, 0xf>(-1, pos);               // wave_shr:1
        const u64 m_bad = __builtin_amdgcn_ballot_w64(
            ovf_solo ||
            (valid && (pos < 0 || pos >= (1 << 30) || d <= -(1 << 30) || d >= (1 << 30) || alen >= 0xFFFFFF)) ||
            (lane > 0 && valid && pos < pos_prev));                        // (the scans below assume sorted positions)
        if (m_bad != 0) { if (lean_row) why = ovf_solo ? 2 : 3; lean_row = false; }
        const u64 m_plain = __builtin_amdgcn_ballot_w64((valid && (!is_snp || (i64)pos + 1 > R64)) || (lane > 0 && valid && pos == pos_prev));
        alen0 = alen;                                // (a shift may cut the allele below)
        altoff = rec.w;
        m_ins = lean_row ? __builtin_amdgcn_ballot_w64(valid && alen0 > 1) : 0;
        issue_allele_bytes();

        if (lean_row && (m_plain == 0 || (A.dbg & GVL_ABL(DBG_ABL_NO_ALLELES)))) {
            // SNPs only, distinct positions inside the contig: whichever way the shift completes (:115-146) or runs
            // out (:200-205) ref_idx lands on ref_start + shift; SNP i sits at pos_i - r0 iff that is inside the row
            a_out = pos - r0;
            applied = valid && pos >= r0 && a_out < L;
            w_i = 1;
            if (!spec_ok) { lean_row = false; why = 4; }          // trailing pad
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
                            if (lane == f) { alen -= skip; a0 += (u32)skip; skip_l = skip; }
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
                for (int it = 0; it < 4 && !stable; ++it) {
                    PM = lean_scan_excl<OpMaxU>(inB ? E : 0, lane, short_scans);
                    PM = PM > ref_idx0 ? PM : ref_idx0;
                    inB = cand && pos >= PM;
                    const u64 m2 = __builtin_amdgcn_ballot_w64(inB);
                    stable = m2 == mB;
                    mB = m2;
                }
                if (!stable) { lean_row = false; why = 5; }
            }
            const int n_i = inB ? pos - PM : 0;
            const int S_i = inB ? OpSat::f(n_i, alen) : 0;
            const int X = lean_scan_excl<OpSat>(S_i, lane, short_scans);
            a_out = OpSat::f(X, n_i);
            applied = inB && a_out < L;                                           // :154-158 break
            w_i = applied ? ((alen < L - a_out) ? alen : L - a_out) : 0;         // :178
            nonsnp = applied && !is_snp;
            dv = cs32 + (u32)E - (u32)(a_out + alen);
            // the walk's state behind the last applied variant, then the tail (:200-255): it must reach L without padding
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
            if (L - out_idx_end > 0 && (i64)(L - out_idx_end) > R64 - (i64)ref_idx_end) { lean_row = false; why = 6; }   // trailing pad
        }
    }
    LEAN_STAMP(4);
    if (!lean_row) {
        LEAN_NOTE(8, 3);
        LEAN_NOTE(9, why);
        if constexpr (RAGL)
            lean_solo_row_at<OH, HAPS>((u64)__builtin_amdgcn_kernarg_segment_ptr(), k, c_s, c_e, l_start, ref_only ? l_end : l_shift, l_oidx, (rc ? 1 : 0) | ((c_ok && o_ok && !ref_only) ? 2 : 0),
                                       (u32)chunk | ((u32)(chunk0 + n_sub - 1) << 16), (LutsLds)&solo_luts, (SoloLdsLds)(SoloLds<false> *)(void *)&solo_all[0], l_o0,
                                       (int)(l_o1 - l_o0 > 0x7FFFFF00ll ? 0x7FFFFF00ll : (l_o1 - l_o0 < 0 ? 0 : l_o1 - l_o0)));
        else
        lean_solo_row<OH, HAPS, CL, ANN>((u64)__builtin_amdgcn_kernarg_segment_ptr(), k, c_s, c_e, l_start, l_shift, l_oidx, (rc ? 1 : 0) | ((c_ok && o_ok) ? 2 : 0),
                                (u32)chunk | ((u32)(chunk0 + n_sub - 1) << 16),
                                (LutsLds)&solo_luts, (SoloLdsLds)(SoloLds<false> *)(void *)&solo_all[0]);
        __builtin_unreachable();     // (the callee ends the wave)
    }

    // ---- phase A: gather the reference runs into the nibble row ------------------------------------------
    // Every read a row with indels needs -- its runs behind the first indel again, the second run of a lane
    // whose 8 bases hold an allele start, the allele bytes that are not inline -- depends on the plan only, so
    // all of them are issued before the first one is waited for: one memory round trip, not three.
    u32 *const row = rows[wave];
    // (LONG: an indel at or in front of the chunk's first base is already in d_init)
    const u64 m_ns = __builtin_amdgcn_ballot_w64(nonsnp && (!LONG || a_out > 0));
    const bool respec = !(m_ns == 0 && d_init == G0 && spec_ok) && !(A.dbg & GVL_ABL(DBG_ABL_NO_REALIGN));     // (not the one run that was read speculatively)
    u32 x[LEAN_STEPS];
    if (!respec) {
        LEAN_NOTE(8, 0);
        const u32 sh = 4u * (G0 & 1u);
#pragma unroll
        for (int s = 0; s < LEAN_STEPS; ++s) x[s] = (u32)(xw[s] >> sh);
    } else {
        // Where do the runs come from?  Indels move a row's sources by a few bases, so almost always they lie
        // inside the window that was read speculatively (+ LEAN_TAIL bases): park that window in the row buffer
        // as it is and let every lane pick its 8 bases at its run's offset -- no second trip to memory.  The
        // test is wave-uniform (a run's offset from the window is a scalar): every run must start inside the
        // window and may not reach more than LEAN_TAIL bases behind the row; and two allele starts less than 8
        // bases apart could share a lane's 8 bases (a lane handles ONE run boundary).
        const int n_dw = (L + 7) >> 3;               // dwords of the row; the tail sits right behind them
        const int rho0 = (int)(d_init - G0);
        bool in_win = spec_ok && rho0 >= 0 && rho0 <= LEAN_TAIL && !(A.dbg & DBG_NO_REALIGN_LDS);
        {
            int a_prev = -8;
            for (u64 m = m_ns; m; m &= m - 1) {
                const int j = __builtin_ctzll(m);
                const int aj = rdl(a_out, j);
                const int rho = (int)((u32)rdl((int)dv, j) - G0);
                in_win = in_win && aj - 7 + rho >= 0 && rho <= LEAN_TAIL && aj - a_prev >= 8;
                a_prev = aj;
            }
        }
        // the run that holds the first of the lane's 8 bases of step s (offset of the last indel at or in front of
        // it) and -- if an allele starts inside the 8 bases -- where, and the run behind that allele
        auto runs_of = [&](const int q, u32 &lo_d, u32 &hi_d, int &cut, bool &multi) {
            lo_d = d_init; hi_d = d_init; cut = 8; multi = false;
            for (u64 m = m_ns; m; m &= m - 1) {
                const int j = __builtin_ctzll(m);
                const int aj = rdl(a_out, j);
                const u32 dj = (u32)rdl((int)dv, j);
                if (q >= aj) { lo_d = dj; hi_d = dj; }
                else if (aj <= q + 7) {
                    if (cut != 8) multi = true;          // a second allele start inside the same 8 bases: base by base
                    else cut = aj - q;
                    hi_d = dj;
                }
            }
        };
        LEAN_NOTE(8, in_win ? 1 : 2);
        if (in_win) {
            const u32 sh = 4u * (G0 & 1u);
#pragma unroll
            for (int s = 0; s < LEAN_STEPS; ++s)
                if (s * 512 < L) row[s * WAVE + lane] = (u32)(xw[s] >> sh);
            if (lane < LEAN_TAIL / 8) row[n_dw + lane] = (u32)(xw_tail >> sh);
            if (lane == 0) row[n_dw + LEAN_TAIL / 8] = 0;
            LEAN_STAMP(11);
            // (one pass over the indels for all four steps, while the window settles in LDS; no two allele starts
            // share a lane's 8 bases here: in_win)
            int rl[LEAN_STEPS], rh[LEAN_STEPS], cut[LEAN_STEPS];
#pragma unroll
            for (int s = 0; s < LEAN_STEPS; ++s) { rl[s] = rho0; rh[s] = rho0; cut[s] = 8; }
            for (u64 m = m_ns; m; m &= m - 1) {
                const int j = __builtin_ctzll(m);
                const int aj = rdl(a_out, j);
                const int rho = (int)((u32)rdl((int)dv, j) - G0);
#pragma unroll
                for (int s = 0; s < LEAN_STEPS; ++s) {
                    const int q = s * 512 + q_lane;
                    if (q >= aj) { rl[s] = rho; rh[s] = rho; }
                    else if (aj <= q + 7) { cut[s] = aj - q; rh[s] = rho; }
                }
            }
            LEAN_STAMP(12);
            wave_lds_fence();
            LEAN_STAMP(13);
            auto pick8 = [&](const int r) -> u32 {
                const u32 lo = row[r >> 3], hi = row[(r >> 3) + 1];
                return __builtin_amdgcn_alignbit(hi, lo, 4u * ((u32)r & 7u));
            };
            const int lim = 8 * n_dw + LEAN_TAIL - 8;    // (lanes behind the end of a short row: keep the reads inside the buffer)
#pragma unroll
            for (int s = 0; s < LEAN_STEPS; ++s) {
                x[s] = 0;
                if (s * 512 < L) {
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
            LEAN_STAMP(14);
            wave_lds_fence();
        } else {
            // the general way: every run read from the packed reference at its own address.  A position inside a
            // long inserted allele has no reference byte behind it (it is overwritten in phase B): clamp the
            // address into the contig so that the read is harmless
            auto clampp = [&](u32 p) { return p < cs32 ? cs32 : (p > ce32 ? ce32 : p); };
            // 8 bases from output position q on, read at q + delta.  `rel` = that position relative to the contig start:
            // negative when q itself lies inside an inserted allele that is longer than the reference in front of it --
            // if ALL 8 bases do (rel <= -8) any address will do; if only some do (-8 < rel < 0) the others are real and an
            // address clamped for the first base would shift them: those lanes build their 8 bases one by one (`mixed`)
            auto gather8 = [&](const int q, const u32 delta, bool &mixed) -> u32 {
                const int rel = (int)((u32)q + delta - cs32);
                mixed = rel < 0 && rel > -8;
                const u32 p = rel < 0 ? cs32 : (rel > R ? ce32 : cs32 + (u32)rel);
                u64 v;
                __builtin_memcpy(&v, A.ref4 + (p >> 1), 8);
                return (u32)(v >> (4u * (p & 1u)));
            };
            u32 y[LEAN_STEPS], z[LEAN_STEPS]; int cuts[LEAN_STEPS]; u32 multis = 0;
#pragma unroll
            for (int s = 0; s < LEAN_STEPS; ++s) {
                y[s] = 0; z[s] = 0; cuts[s] = 8;
                if (s * 512 < L && !(A.dbg & GVL_ABL(DBG_ABL_NO_LOADS))) {
                    u32 lo_d, hi_d; bool multi;
                    runs_of(s * 512 + q_lane, lo_d, hi_d, cuts[s], multi);
                    bool mixed_lo, mixed_hi;
                    y[s] = gather8(s * 512 + q_lane, lo_d, mixed_lo);
                    z[s] = gather8(s * 512 + q_lane, hi_d, mixed_hi);
                    if (multi || mixed_lo || mixed_hi) multis |= 1u << s;
                }
            }
#pragma unroll
            for (int s = 0; s < LEAN_STEPS; ++s) {
                const u32 lowm = cuts[s] >= 8 ? 0xFFFFFFFFu : ((1u << (4 * cuts[s])) - 1u);
                x[s] = (y[s] & lowm) | (z[s] & ~lowm);
            }
            if (__builtin_amdgcn_ballot_w64(multis != 0)) {
#pragma unroll 1
                for (int s = 0; s < LEAN_STEPS; ++s) {
                    if ((multis >> s) & 1u) {
                        const int q = s * 512 + q_lane;
                        u32 v = 0;
#pragma unroll 1
                        for (int i = 0; i < 8; ++i) {
                            u32 dd = d_init;
                            for (u64 m = m_ns; m; m &= m - 1) {
                                const int j = __builtin_ctzll(m);
                                if (q + i >= rdl(a_out, j)) dd = (u32)rdl((int)dv, j);
                            }
                            const u32 p = clampp((u32)(q + i) + dd);
                            const u32 b = (A.dbg & GVL_ABL(DBG_ABL_NO_LOADS)) ? 0u : (u32)A.ref4[p >> 1];
                            v |= ((b >> (4u * (p & 1u))) & 0xFu) << (4 * i);
                        }
                        x[s] = v;     // (x[] is indexed by a loop variable here: rare path, the spill is its own)
                    }
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < LEAN_STEPS; ++s)
        if (s * 512 < L) row[s * WAVE + lane] = x[s];
    wave_lds_fence();
    LEAN_STAMP(5);

    // ---- phase B: SNPs and allele bytes ---------------------------------------------------------------------
    if (applied && w_i > 0 && skip_l == 0 && (!LONG || a_out >= 0)) row_set_nibble(row, a_out, ref4_nibble(inl));      // an allele's first byte is inline
    if (m_ins && !(A.dbg & GVL_ABL(DBG_ABL_NO_REALIGN))) {
        // byte i (>= 1) of variant j's allele lands at a_out_j + i - skip_j if the variant is applied and the byte is
        // among the w_j the row has room for
        auto place = [&](const int t, const int owner, const int i, const u32 b) {
            const int ii = i - bperm(owner, skip_l);
            const int o_w = bperm(owner, w_i), o_a = bperm(owner, a_out);
            if (t < pb_total && ii >= 0 && ii < o_w && (!LONG || (u32)(o_a + ii) < (u32)L))     // (w_i is 0 unless applied; LONG: the chunk's part of the allele)
                row_set_nibble(row, o_a + ii, ref4_nibble(b));
        };
        place(lane, pb_owner, pb_i, pb_v);
        for (int t0 = WAVE; t0 < pb_total; t0 += WAVE) {        // (more than 64 such bytes in one row: rare)
            int owner, i;
            const u8 *src = allele_byte_of(t0 + lane < pb_total ? t0 + lane : 0, owner, i);
            const u32 b = t0 + lane < pb_total ? (u32)*src : 0u;
            place(t0 + lane, owner, i, b);
        }
    }
    wave_lds_fence();
    LEAN_STAMP(6);
    if (HAPS) {
        // a nibble 0 in the finished row = a byte that is neither ACGT nor N: only the byte reference can write it
        bool other = false;
#pragma unroll
        for (int s = 0; s < LEAN_STEPS; ++s) {
            if (s * 512 + q_lane < L) {
                u32 v = row[s * WAVE + lane];
                const int n_in = L - (s * 512 + q_lane);                    // bases of this dword inside the row
                if (n_in < 8) v |= 0xFFFFFFFFu << (4 * n_in);
                other = other || (((v - 0x11111111u) & ~v & 0x88888888u) != 0u);
            }
        }
        if (__builtin_amdgcn_ballot_w64(other)) {
            if constexpr (RAGL)
                lean_solo_row_at<OH, HAPS>((u64)__builtin_amdgcn_kernarg_segment_ptr(), k, c_s, c_e, l_start, ref_only ? l_end : l_shift, l_oidx, (rc ? 1 : 0) | (ref_only ? 0 : 2),
                                           (u32)chunk | ((u32)(chunk0 + n_sub - 1) << 16), (LutsLds)&solo_luts, (SoloLdsLds)(SoloLds<false> *)(void *)&solo_all[0], l_o0, Lrow);
            else
            lean_solo_row<OH, HAPS, CL, ANN>((u64)__builtin_amdgcn_kernarg_segment_ptr(), k, c_s, c_e, l_start, l_shift, l_oidx, (rc ? 1 : 0) | 2,
                                    (u32)chunk | ((u32)(chunk0 + n_sub - 1) << 16),
                                    (LutsLds)&solo_luts, (SoloLdsLds)(SoloLds<false> *)(void *)&solo_all[0]);
            __builtin_unreachable();
        }
    }

    // ---- phase C: stream -------------------------------------------------------------------------------------
    if constexpr (!LONG) __builtin_amdgcn_s_setprio(0);
    // (LONG: the chunk's bases sit at [lo, lo + L) of the row, at [Lrow - lo - L, Lrow - lo) of a reverse-complemented one)
    const i64 row0 = (RAGL ? l_o0 : (i64)k * Lrow) + (LONG ? (rc ? Lrow - lo - L : lo) : 0);
    u8 *const oh_row = OH ? A.onehot + row0 * 4 : nullptr;
    u8 *const hap_row = HAPS ? A.haps + row0 : nullptr;
    const u32 sel = rc ? 0x0c0c0001u : 0x0c0c0100u;                      // v_perm: 16 bits, byte-swapped for RC
    const u32 tbase = rc ? 256u : 0u;
    // forward: group p lands at base p (bytes) / 4 p (one-hot); reverse-complement: at L - 4 - p
    const i64 hp_lane = rc ? ((i64)L - 4 - 4 * (i64)lane) : 4 * (i64)lane;
    const i64 st_lane = 4 * hp_lane;
    const int hp_step = rc ? -TRIP : TRIP;
    const int st_step = 4 * hp_step;
    const unsigned short *row16 = reinterpret_cast<const unsigned short *>(row);
    const u32 lane4 = (u32)lane * GROUP;
    // Whole trips (L a multiple of 256: every lane stores in every trip) in groups of 4: all 16-bit reads first, then all
    // table lookups, then the stores -- three LDS round trips per 4 trips instead of two per trip.
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
    if constexpr (CL) {
        // channel-major: plane c of row k at onehot + (4 k + c) Lrow; the chunk's bases at the same offset of every plane
        if (!(A.dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
            u8 *const cl_base = A.onehot + (i64)k * 4 * Lrow + (rc ? Lrow - lo - L : lo);
            (void)stream_onehot_cl<LEAN_MAX_TRIPS * TRIP>(row, lut, tbase, rc, L, (i64)Lrow, cl_base, lane);
            if (HAPS) {
#pragma unroll
                for (int u = 0; u < LEAN_MAX_TRIPS; ++u) {
                    if (u * TRIP < L) {
                        const u32 rr = __builtin_amdgcn_perm(0u, (u32)row16[u * WAVE + lane], sel);
                        const u32 hb = (u32)blut[tbase + (rr & 0xFFu)] | ((u32)blut[tbase + (rr >> 8)] << 16);
                        if (u * TRIP + (int)lane4 < L) store_u32_unaligned(hap_row + hp_lane + (i64)u * hp_step, hb);
                    }
                }
            }
        }
    } else if ((L & (4 * TRIP - 1)) == 0 && !(A.dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
        stream4(0);
        if (L > 4 * TRIP) stream4(4);
    } else if constexpr (RAGL) {
        // a chunk of any length (a ragged row's last one): fg whole 4-base groups -- group g at base 4 g of the chunk, or at L - 4 - 4 g
        // of a reverse-complemented one -- then the last L & 3 bases dword by dword / byte by byte, by the lane that owns their
        // group (a reverse-complemented chunk's are its FIRST bases): recon_lean_rows_kernel's ragged phase C
        const int fg = L >> 2, rem = L & 3;
        if (!(A.dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
#pragma unroll
            for (int u = 0; u < LEAN_MAX_TRIPS; ++u) {
                if (u * WAVE < fg || (rem > 0 && u * WAVE == fg)) {
                    const u32 r = row16[u * WAVE + lane];
                    const u32 rr = __builtin_amdgcn_perm(0u, r, sel);
                    uint2 a = make_uint2(0u, 0u), b = make_uint2(0u, 0u);
                    u32 hb = 0;
                    if (OH) { a = lut[tbase + (rr & 0xFFu)]; b = lut[tbase + (rr >> 8)]; }
                    if (HAPS) hb = (u32)blut[tbase + (rr & 0xFFu)] | ((u32)blut[tbase + (rr >> 8)] << 16);
                    if (u * WAVE + lane < fg) {
                        if (OH) {
                            u32x4_a4 o = {a.x, a.y, b.x, b.y};
                            store_oh16(oh_row + st_lane + (i64)u * st_step, o);
                        }
                        if (HAPS) store_u32_unaligned(hap_row + hp_lane + (i64)u * hp_step, hb);
                    }
                    if (rem > 0 && (fg >> 6) == u) {
                        const bool mine = lane == (fg & (WAVE - 1));
                        const i64 t0 = rc ? 0 : 4 * (i64)fg;
                        const u32 od[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            if (j < rem) {
                                const int src_j = rc ? 4 - rem + j : j;
                                if (OH) {
                                    const u32 dwv = src_j == 0 ? od[0] : src_j == 1 ? od[1] : src_j == 2 ? od[2] : od[3];
                                    if (mine) __builtin_nontemporal_store(dwv, reinterpret_cast<u32 *>(oh_row + 4 * (t0 + j)));
                                }
                                if (HAPS) {
                                    if (mine) hap_row[t0 + j] = (u8)(hb >> (8 * src_j));
                                }
                            }
                        }
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int u = 0; u < LEAN_MAX_TRIPS; ++u) {
            if (u * TRIP < L) {
                const u32 r = row16[u * WAVE + lane];
                const u32 rr = __builtin_amdgcn_perm(0u, r, sel);
                if (u * TRIP + (int)lane4 < L && !(A.dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
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
    if constexpr (ANN) {
        // ---- annotations of the chunk: per output base {variant index or -1, reference coordinate} (src/reconstruct/mod.rs:160-190: reference
        // bases carry their own coordinate, allele bytes their variant's index and position).  Forward position p of the chunk lies in the
        // allele of entry j iff a_out_j <= p < a_out_j + w_j, else in the reference run behind the last indel at or in front of it.  A lane
        // takes four consecutive output positions per trip; a reverse-complemented row's annotations are reversed (src/reverse.rs:25-38).
        if (!(A.dbg & GVL_ABL(DBG_ABL_NO_STORES))) {
            int *const av_row = A.av + row0, *const ap_row = A.ap + row0;
            const u64 m_app = __builtin_amdgcn_ballot_w64(applied && w_i > 0);
            const u64 m_nsa = __builtin_amdgcn_ballot_w64(nonsnp);
            const int nba = L >> 2;                   // (L is a multiple of 4: fixed-length rows of 4 k bases, chunks of 2048)
#pragma unroll 1
            for (int u = 0; u * WAVE < nba; ++u) {
                const int t = u * WAVE + lane;
                const int q0 = 4 * t;                                     // the lane's output positions q0 .. q0 + 3
                const int p0 = rc ? L - 4 - q0 : q0;                      // ... hold forward positions p0 .. p0 + 3 (rc: in reverse)
                const int ts = rc ? L - TRIP * (u + 1) : TRIP * u, te = ts + TRIP;      // the trip's forward range
                u32 Dbase = d_init;
                u64 touch = 0;
                for (u64 m = m_app | m_nsa; m; m &= m - 1) {
                    const int j = __builtin_ctzll(m);
                    const int a = rdl(a_out, j);
                    if (a >= te) break;                                  // (sorted: the rest start behind the trip)
                    const bool nsj = ((m_nsa >> j) & 1ull) != 0;
                    if (nsj && a <= ts) Dbase = (u32)rdl((int)dv, j);
                    if ((((m_app >> j) & 1ull) && a + rdl(w_i, j) > ts) || (nsj && a > ts)) touch |= 1ull << j;
                }
                u32 D[4] = {Dbase, Dbase, Dbase, Dbase};
                int id[4] = {-1, -1, -1, -1}, ps[4] = {0, 0, 0, 0};
                for (u64 m = touch; m; m &= m - 1) {
                    const int j = __builtin_ctzll(m);
                    const int a = rdl(a_out, j), w = ((m_app >> j) & 1ull) ? rdl(w_i, j) : 0, idj = rdl(e_vid, j), pj = rdl(e_pos, j);
                    const u32 dj = (u32)rdl((int)dv, j);
                    const bool nsj = ((m_nsa >> j) & 1ull) != 0;
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
            }
        }
    }
#ifdef GVL_DIAG
    if (A.stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); LEAN_STAMP(7); LEAN_NOTE(9, m_ins != 0); }
#endif
    if constexpr (LONG) wave_lds_fence();        // (the next chunk's entries go where this chunk's nibbles are being read)
    }
}


// ---- chunk plans of rows of several chunks (BASELINE config 4) -----------------------------------------------------------------
// recon_lean_kernel<.., LONG> gives every pair of 2048-base chunks of a row its own wave, and without a plan each of those waves
// replays the row's walk up to its chunk -- 1.5-3 trips of 64 variants with their scans, about 40 % of the kernel's instructions on
// BASELINE config 4's 131 072-base rows.  hap_plan_kernel walks every row ONCE, a wave per row -- the same trips: src/reconstruct/
// mod.rs:85-198 restated exactly as in recon_lean_kernel's LONG branch -- and leaves per (row, chunk) what the chunk's wave needs:
// where its window starts in the packed reference (the delta behind the last indel whose allele starts at or in front of the chunk's
// first base) and the applied variants whose allele bytes fall into the chunk, in the form the kernel's phases A / B read (gvl_internal.inc:
// HP_STRIDE_DW dwords per (row, chunk)).  A chunk the plan cannot express -- more than HP_ENT entries, a walk the scans give up on, a
// tail that would need padding -- is flagged: its wave then walks the row itself, exactly as without a plan, and sends what it cannot
// take to the all-purpose body.  Made once per epoch for every row of the epoch (the native loader; gvl_hap_plan for any other caller).
__global__ __launch_bounds__(LEAN_THREADS) void hap_plan_kernel(const LeanArgs A, u32 *const plan) {
    constexpr int CH = LEAN_MAX_TRIPS * TRIP;
    __shared__ u32 s_cnt[LEAN_WAVES][HP_MAX_CHUNKS];        // entries of the row's chunks so far
    __shared__ u32 s_dcell[LEAN_WAVES][HP_MAX_CHUNKS];      // chunk c: the delta behind the last indel whose allele starts in (lo_{c-1}, lo_c]
    __shared__ u32 s_dval[LEAN_WAVES][HP_MAX_CHUNKS / 32];  // ... and whether there is one
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = rfl(tid >> 6);
    const int k = (int)blockIdx.x * LEAN_WAVES + wave;
    if (k >= A.n_rows) return;
    const int chunks = A.chunks;
    const int Lrow = A.L;
    u32 *const cnt = s_cnt[wave];
    u32 *const dcell = s_dcell[wave];
    u32 *const dval = s_dval[wave];
    for (int c = lane; c < chunks; c += WAVE) cnt[c] = 0;
    for (int c = lane; c < (chunks + 31) / 32; c += WAVE) dval[c] = 0;
    u32 *const prow = plan + (i64)k * chunks * (i64)HP_STRIDE_DW;

    const int query = A.ploidy_shift >= 0 ? (k >> A.ploidy_shift) : (int)((u32)k / (u32)A.ploidy);
    const int *p_reg = A.regions + (i64)query * A.regions_stride;
    const int l_c = rfl(p_reg[0]), l_start = rfl(p_reg[1]);
    const int l_shift = rfl(A.shifts[k]);
    const i64 l_oidx = rfl64(A.geno_offset_idx[k]);
    const bool c_ok = (u32)l_c < (u32)A.n_contigs;
    const bool o_ok = l_oidx >= 0 && l_oidx < A.n_geno_offsets;
    const i64 c_s = rfl64(A.ref_offsets[c_ok ? l_c : 0]), c_e = rfl64(A.ref_offsets[(c_ok ? l_c : 0) + 1]);
    const i64 o_s = rfl64(A.go_starts[o_ok ? l_oidx : 0]);
    const i64 nv64 = rfl64(A.go_stops[o_ok ? l_oidx : 0]) - o_s;
    const i64 R64 = c_e - c_s;
    const u32 cs32 = (u32)c_s;
    bool ok = c_ok && o_ok && l_start >= 0 && l_start < (1 << 30) && l_shift >= 0 && l_shift < (1 << 30) && R64 >= 0 && R64 < (1ll << 31) &&
              !(A.dbg & DBG_LEAN_SOLO) && A.grec != nullptr && nv64 >= 0 && nv64 < (1ll << 30);
    const int n_var = ok ? (int)nv64 : 0;
    wave_lds_fence();

    int rem = l_shift, ref_idx0 = l_start, pm_carry = l_start, x_carry = 0, pos_carry = -1;
    bool ended = false;
    int ref_idx_end = l_start, out_idx_end = 0, ao_last = -1;
    const i32x4 rec_none = {0, 0, 0, 0};
    i32x4 nxt = rec_none;
    // (a keep mask hides variants from the walk, src/reconstruct/mod.rs:86-90: the plan is then THIS mask's)
    const bool has_keep = A.keep != nullptr && A.keep_offsets != nullptr;
    const i64 l_ko = has_keep ? rfl64(A.keep_offsets[k]) : 0;
    u32 nxt_keep = 1;
    if (lane < n_var) {
        nxt = *reinterpret_cast<const i32x4 *>(A.grec + (o_s + lane));
        if (has_keep) nxt_keep = (u32)A.keep[l_ko + lane];
    }
#pragma unroll 1
    for (int tb = 0; tb < n_var && ok && !ended; tb += WAVE) {
        const i32x4 r = nxt;
        const bool kept = nxt_keep != 0;
        nxt = rec_none;
        nxt_keep = 1;
        if (tb + WAVE + lane < n_var) {
            nxt = *reinterpret_cast<const i32x4 *>(A.grec + (o_s + tb + WAVE + lane));
            if (has_keep) nxt_keep = (u32)A.keep[l_ko + tb + WAVE + lane];
        }
        const bool in_row = tb + lane < n_var;
        const bool v = in_row && kept;
        const int pos = r.x, d = r.y, vi = r.w;
        int al = (int)((u32)r.z >> 8);
        const int al0 = al;
        const u32 in_ = (u32)r.z & 0xFFu;
        int skip = 0;
        const int pos_prev = dpp_mov<0x138, 0xf>(pos_carry, pos);           // wave_shr:1 (lane 0: the trip before)
        const u64 m_bad = __builtin_amdgcn_ballot_w64(
            in_row && (pos < 0 || pos >= (1 << 30) || d <= -(1 << 30) || d >= (1 << 30) || al >= 0xFFFFFF || pos < pos_prev));
        if (m_bad) { ok = false; break; }
        pos_carry = rdl(pos, WAVE - 1);
        const int E = pos - (d < 0 ? d : 0) + 1;                            // v_ref_end, :96
        const bool snp = d == 0 && al == 1;
        const u64 m_span = __builtin_amdgcn_ballot_w64(v && pos < l_start && d < 0 && E >= l_start);      // :99-102
        if (m_span) { ref_idx0 = rdl(E, 63 - __builtin_clzll(m_span)); pm_carry = ref_idx0; ref_idx_end = ref_idx0; }
        bool cand = v && pos >= l_start;
        if (rem > 0) {      // shift consumption (:115-146)
            const int base = ref_idx0;
            const u64 m_t = __builtin_amdgcn_ballot_w64(cand && pos >= base && (pos - base) + al >= rem);
            if (m_t == 0) {
                cand = false;
            } else {
                const int f = __builtin_ctzll(m_t);
                const int dist = rdl(pos, f) - base;
                if (dist >= rem) {
                    ref_idx0 = base + rem;
                    cand = cand && lane >= f;
                } else {
                    const int sk = rem - dist;
                    if (sk == rdl(al, f)) {
                        ref_idx0 = rdl(E, f);
                        cand = cand && lane > f;
                    } else {
                        ref_idx0 = rdl(pos, f);
                        cand = cand && lane >= f;
                        if (lane == f) { al -= sk; skip = sk; }
                    }
                }
                rem = 0;
                pm_carry = ref_idx0; ref_idx_end = ref_idx0;
            }
        }
        bool inB = cand;                                                    // first ALT wins (:108-110)
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
            if (!stable) { ok = false; break; }
        }
        const int n_i = inB ? pos - PM : 0;
        const int S_i = inB ? OpSat::f(n_i, al) : 0;
        int x_incl;
        const int X = OpSat::f(x_carry, wave_scan_exclusive<OpSat>(S_i, x_incl));
        const int ao = OpSat::f(X, n_i);                                     // allele start, row coordinates
        const bool app = inB && ao < Lrow;                                   // :154-158 break
        const int wi = app ? ((al < Lrow - ao) ? al : Lrow - ao) : 0;       // :178
        const bool ns = app && !snp;
        const u64 m_inB = __builtin_amdgcn_ballot_w64(inB);
        const u64 m_app = __builtin_amdgcn_ballot_w64(app);
        if (m_inB != m_app) ended = true;
        if (m_app) {
            const int last = 63 - __builtin_clzll(m_app);
            ref_idx_end = rdl(E, last);
            ao_last = rdl(ao, last);
            out_idx_end = ao_last + rdl(wi, last);
        }
        const u32 dvr = cs32 + (u32)E - (u32)(ao + al);                     // delta behind this variant, row coordinates
        // ---- entries: variant -> the chunks its allele bytes fall into (c0 .. c1; almost always one)
        const int c0 = app ? ao / CH : 0, c1 = app ? (ao + wi - 1) / CH : 0;
        const u32 e_flags = in_ | (snp ? 256u : 0u);
        const u32 e_alt = (app && al0 > 1) ? (u32)(u64)A.alt_offsets[vi] : 0u;     // (only an allele with bytes behind its first needs its offset)
        auto put = [&](const int c, const int slot) {
            const int lo_c = c * CH;
            i32x4 *const dst = reinterpret_cast<i32x4 *>(prow + (i64)c * HP_STRIDE_DW + 4 + 8 * slot);
            const i32x4 a = {ao - lo_c, wi, al, al0};
            const i32x4 b = {(int)(dvr + (u32)lo_c), (int)e_flags, (int)e_alt, skip};
            dst[0] = a; dst[1] = b;
            *reinterpret_cast<int2 *>(prow + (i64)c * HP_STRIDE_DW + HP_ANNEX_DW + 2 * slot) = make_int2(vi, pos);     // (annotated rows)
        };
        // an allele that reaches into the chunks behind its own: it is their FIRST entry (entries are sorted and do not overlap)
        if (app && c1 > c0) {
            for (int c = c0 + 1; c <= c1; ++c) { put(c, 0); cnt[c] = 1; }
        }
        wave_lds_fence();
        // the chunk an allele starts in: slot = entries of the chunk so far + rank among this trip's lanes of the same chunk
        const u64 below = (1ull << lane) - 1ull, upto = (2ull << lane) - 1ull;
        const u64 mb = m_app & below;
        const int c0_prev = bperm(mb ? 63 - __builtin_clzll(mb) : 0, c0);
        const bool is_head = app && (mb == 0 || c0_prev != c0);
        const u64 m_head = __builtin_amdgcn_ballot_w64(is_head);
        const u64 hm = m_head & upto;
        const int head_lane = hm ? 63 - __builtin_clzll(hm) : 0;
        const int rank = __builtin_popcountll(mb & ~((1ull << head_lane) - 1ull));
        const int slot = app ? (int)cnt[c0] + rank : 0;
        if (app && slot < HP_ENT) put(c0, slot);
        const u64 ma = m_app & ~upto;
        const int c0_next = bperm(ma ? __builtin_ctzll(ma) : 0, c0);
        const bool is_tail = app && (ma == 0 || c0_next != c0);
        wave_lds_fence();                                                    // (every lane has read its chunk's count)
        if (is_tail) cnt[c0] = (u32)(slot + 1);
        // the delta in front of a chunk: behind the LAST indel whose allele starts at or in front of the chunk's first base
        const int cc = (ao + CH - 1) / CH;                                   // the first chunk that begins at or behind this allele's start
        const u64 m_nsl = __builtin_amdgcn_ballot_w64(ns);
        const u64 mn = m_nsl & ~upto;
        const int cc_next = bperm(mn ? __builtin_ctzll(mn) : 0, cc);
        if (ns && cc < chunks && (mn == 0 || cc_next != cc)) {
            dcell[cc] = dvr;
            __hip_atomic_fetch_or(&dval[cc >> 5], 1u << (cc & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        wave_lds_fence();
        if (tb + WAVE < n_var) {        // carries (pm_incl: the scan of the last fixed-point round = the final mask's)
            const int mx = rdl(pm_incl, WAVE - 1);
            pm_carry = mx > pm_carry ? mx : pm_carry;
            x_carry = OpSat::f(x_carry, rdl(x_incl, WAVE - 1));
        }
    }
    if (ok && rem > 0) {                              // the shift never completed: nothing was applied
        const i64 t = (i64)ref_idx0 + rem;
        ref_idx_end = (int)(t < R64 ? t : R64);
    }
    // ---- per chunk: its delta (a running "last one set" over the chunks), flags, header
    u32 d_run = cs32 + (u32)(rem > 0 ? ref_idx_end : ref_idx0);
    for (int cb = 0; cb < chunks; cb += WAVE) {
        const int c = cb + lane;
        const bool inr = c < chunks;
        const bool hv = inr && ((dval[c >> 5] >> (c & 31)) & 1u) != 0;
        const u32 dc = hv ? dcell[c] : 0u;
        const u64 mv = __builtin_amdgcn_ballot_w64(hv);
        const u64 mle = mv & ((2ull << lane) - 1ull);
        const u32 d_own = (u32)bperm(mle ? 63 - __builtin_clzll(mle) : 0, (int)dc);
        const u32 d0 = mle ? d_own : d_run;
        if (mv) d_run = (u32)rdl((int)dc, 63 - __builtin_clzll(mv));
        if (inr) {
            const int lo_c = c * CH;
            const int Lc = Lrow - lo_c < CH ? Lrow - lo_c : CH;
            const int hi_c = lo_c + Lc;
            const int n = (int)cnt[c];
            bool okc = ok && n <= HP_ENT && Lc > 0;
            // a walk that ran to its end in front of the chunk's end: the tail (:200-255) must reach it without padding
            if (!ended && !(ao_last >= hi_c) && hi_c - out_idx_end > 0 && (i64)(hi_c - out_idx_end) > R64 - (i64)ref_idx_end) okc = false;
            const u32 G0 = d0 + (u32)lo_c;
            const int rel0 = (int)(G0 - cs32);
            const bool spec = okc && rel0 >= 0 && (i64)rel0 + Lc <= R64;
            const i32x4 h = {(int)G0, (int)((u32)(n > 255 ? 255 : n) | (okc ? 0x100u : 0u) | (spec ? 0x200u : 0u)), 0, 0};
            *reinterpret_cast<i32x4 *>(prow + (i64)c * HP_STRIDE_DW) = h;
        }
    }
}
