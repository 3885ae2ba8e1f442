// gvl_internal.inc -- what the translation units of libgvl_hip.so share: the kernel-argument structs the host code
// fills, the launch constants the dispatch needs, and the internal host interface (namespace gvli; nothing here is exported
// by name -- the C-ABI is include/gvl_hip.h).  Included first by every .hip file of csrc/:
//   gvl_hip.hip        C-ABI entry points, dispatch, small kernels (diffs / keep mask / packers / rc / one-hot / request prep),
//                      the native batch loop
//   gvl_recon.hip      the all-purpose kernel (reconstruct_kernel: 12 instantiations)
//   gvl_lean.hip       recon_lean_kernel (a wave per row; long rows by chunks)
//   gvl_lean_pipe.hip  recon_lean_rows_kernel (one grid over a group of batches)
//   gvl_tracks.hip     track kernels (painter, realignment, row plans) and their entry points
//   gvl_svar2.hip      the SVAR2 two-source provider: merge of a batch's var_key / dense channels into a per-batch sparse table
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <new>
#include <type_traits>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "gvl_hip.h"


namespace gvli {

typedef long long i64;
typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned char u8;
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int WAVE = 64;
constexpr int WG_WAVES = 8;               // one wave per row, 8 rows per workgroup
constexpr int WG_THREADS = WAVE * WG_WAVES;
constexpr int GROUP = 4;                   // bases per lane per trip
constexpr int TRIP = WAVE * GROUP;         // 256 bases per wave trip
enum { OH_NONE = 0, OH_LC = 1, OH_CL = 2 };
constexpr int LEAN_WAVES = 4;
constexpr int LEAN_THREADS = LEAN_WAVES * WAVE;
constexpr int LEAN_MAX_TRIPS = 8;            // rows up to 2048 bases
constexpr int PIPE_MAX_ROWS = 32;            // recon_lean_rows_kernel: rows per wave (a bit per row in the deferred-rows mask)
constexpr int PIPE_RAG_MAXT = 10;            // ... trips of 256 bases of its ragged rows (2560 bases)
// Chunk plans of rows of several chunks (hap_plan_kernel, gvl_lean.inc): per (row, chunk) a block of HP_STRIDE_DW dwords --
// {position of the chunk's first base in the packed reference, entries | flags << 8, 0, 0} and up to HP_ENT entries of 8 dwords
// (the applied variants whose allele bytes fall into the chunk, chunk coordinates); flag 1 = the chunk can be written from its
// plan (else its wave walks the row's variants itself, as without a plan), flag 2 = its window lies inside the contig.
// Round 6: behind the entries an annex of 2 dwords per entry {variant index, position}: what annotated rows need next to an entry
// (read by recon_lean_kernel<.., ANN> only).
constexpr int HP_ENT = 8;
constexpr int HP_ANNEX_DW = 4 + 8 * HP_ENT;        // where the annex begins inside a block
constexpr int HP_STRIDE_DW = 4 + 8 * HP_ENT + 2 * HP_ENT;
constexpr int HP_MAX_CHUNKS = 512;           // rows of more chunks are not planned (a wave's LDS tables)
inline i64 hap_plan_bytes(i64 n_rows, i64 chunks) { return n_rows * chunks * (i64)HP_STRIDE_DW * 4; }

// GVL_DBG bits (the environment's value, or gvl_set_debug_flags): test and diagnostic switches, most of which take away one way
// a row can reach its output so that the GPU suite can be run down every path.  The values are ABI: tests, tools and the Python
// layer pass them as integers.
enum DbgBit : int {
    DBG_ABL_NO_VARIANTS  = 1,           // [ablation] every row as if it had no variants
    DBG_ABL_NO_STORES    = 2,           // [ablation] no output stores
    DBG_ABL_NO_LOADS     = 4,           // [ablation] no reference loads
    DBG_SCALAR_WALK      = 8,           // every row through the scalar walk (haplotypes and tracks); no track row plans
    DBG_NO_GENO_REC      = 16,          // ignore gvl_static.geno_rec (records come from geno_v_idxs -> vrec)
    DBG_NO_SNP_PLAN      = 32,          // no scan-free plan for SNP-only rows (they join the packed plan)
    DBG_NO_SLOT_REC      = 64,          // ignore gvl_static.slot_rec (rows find their records through the CSR)
    DBG_NO_SPEC_REF      = 128,         // no speculative reference reads in front of the plan
    DBG_NO_FRONT         = 256,         // a mixed ragged launch's long rows by the wave that meets them, chunk after chunk (no front
                                        // workgroups: lean_solo_rows' crews); all-purpose kernel: its per-workgroup time stamps
    DBG_NO_PACKABLE      = 512,         // no packable rows at all (every row runs the per-wave scans)
    DBG_NO_BUCKET_INDEX  = 1024,        // the painter ignores the per-list bucket index (exact 64-ary searches per chunk)
    DBG_DIFFS_WAVE_ROWS  = 2048,        // length deltas (get_diffs_sparse, ragged sizing) always one wave per row
    DBG_PAINT_TIMELINE   = 4096,        // the painter records its per-phase time stamps (gvl_diag_set_stamps)
    DBG_PAINT_LDS_IMAGE  = 8192,        // the painter always paints an LDS image (no start-bitmap lookup for non-overlapping candidates)
    DBG_NO_LEAN          = 16384,       // no lean kernel: the all-purpose kernel over every row (tested through the route masks only)
    DBG_LEAN_SOLO        = 32768,       // the lean kernels hand EVERY row to their solo general path (per-wave scans from the byte reference)
    DBG_NO_REALIGN_LDS   = 65536,       // the lean kernels re-read the runs of a row with indels from memory (no re-alignment in LDS)
    DBG_TRACK_SIZING_PER_BATCH = 131072,    // the native loop sizes the scratch tracks per batch (not once per epoch)
    DBG_ABL_NO_REALIGN   = 262144,      // [ablation] the lean kernel without re-alignment (WRONG output for rows with indels)
    DBG_ABL_NO_ALLELES   = 524288,      // [ablation] the lean kernel without allele bytes, and no scan plan (WRONG output for indels)
    DBG_NO_LEAN_LONG     = 1048576,     // rows longer than one chunk never take the lean kernel: the all-purpose kernel
    DBG_NO_REALIGN_WINDOW = 2097152,    // realignment from intervals never uses its window (every value looked up in the interval list)
    DBG_NO_FUSED_TRACKS  = 4194304,     // tracks are always painted into the scratch track first (no realignment straight from intervals)
    DBG_ABL_TRACK_WALK   = 8388608,     // [ablation] realign_tracks_kernel stops behind the walk (NO output)
    DBG_ABL_TRACK_WINDOW = 16777216,    // [ablation] realign_tracks_kernel stops behind the window build (NO output)
    DBG_PIPE_ALWAYS      = 33554432,    // rows of one chunk always take the pipelined kernel, with as few workgroups as 32 rows per wave allow
    DBG_PIPE_NEVER       = 67108864,    // rows of one chunk never take the pipelined kernel (nor its channel-major / annotated / keep-mask forms)
    DBG_RAGGED_PER_BATCH = 134217728,   // the native loop sizes ragged rows per batch (not per epoch or group)
    DBG_NO_TRACK_PLANS   = 268435456,   // no track row plans (track_plan_kernel): every chunk-wave walks its row itself
    DBG_NO_HAP_PLANS     = 536870912,   // rows of several chunks go without chunk plans (hap_plan_kernel): every chunk-wave walks its row
    DBG_ROUND4_ROUTES    = 1073741824,  // round 4's routing of the other output modes: channel-major one-hot, keep masks, annotations,
                                        // get_reference and the fast track kernel run the all-purpose (general) kernel
    DBG_CHUNK_LIST       = (int)0x80000000u,    // ragged track rows of several chunks through their chunk list (1-D launches) instead of the
                                        // rows x chunks grid with early exit; gvl_set_debug_flags(INT_MIN | ...) or GVL_DBG=2147483648
};
// The [ablation] bits change the output: they exist in -DGVL_DIAG builds only (tools/ablate.sh builds one next to the shipped
// library).  The shipped library masks them off on the host (debug_flags) and compiles their tests out of the kernels
// (GVL_ABL(x) = 0): it has no mode that returns wrong bytes.
constexpr int DBG_ABLATIONS = DBG_ABL_NO_VARIANTS | DBG_ABL_NO_STORES | DBG_ABL_NO_LOADS | DBG_ABL_NO_REALIGN | DBG_ABL_NO_ALLELES |
                              DBG_ABL_TRACK_WALK | DBG_ABL_TRACK_WINDOW;
#ifdef GVL_DIAG
#define GVL_ABL(x) (x)
#else
#define GVL_ABL(x) 0
#endif

struct ReconArgs {
    // static
    const u8 *ref; i64 ref_len; const i64 *ref_offsets;
    const gvl_vrec *vrec; const i64 *alt_offsets; const u8 *alt_alleles; i64 alt_len;
    i64 n_variants;
    const i64 *go_starts; const i64 *go_stops; const int *geno_v_idxs; const gvl_grec *grec;
    const gvl_srec *srec;   // slot-major records (nullable): 8 per genotype slot, no CSR hop
    int n_contigs; i64 n_geno_offsets;
    // batch
    const int *regions; i64 regions_stride; const int *shifts; const i64 *geno_offset_idx;
    const u8 *keep; const i64 *keep_offsets; const u8 *to_rc; const i64 *out_offsets;
    i64 fixed_len;      // >= 0 or -1
    i64 n_rows; int ploidy; int ploidy_shift; int chunk_len;
    int dbg;
    int ref_only;       // get_reference mode: no variants, shift 0, row len from out_offsets
    u32 pad;
    u32 oh_cl;          // the one-hot output is channel-major (rows, 4, L) (GVL_ONEHOT_CL)
    // out
    u8 *haps; u8 *onehot; int *av; int *ap; i64 *out_offsets_w;
    u64 *stamps;        // diagnostic builds (-DGVL_DIAG): per-workgroup phase time stamps
    int *async_err;     // host-mapped word: set when the launch finds a row longer than the max_row_len hint
    const u8 *ref4;     // nibble-packed reference (gvl_static.ref4): read by recon_lean_kernel only
    const u32 *hplan;   // rows of several chunks: the caller's row plans (gvl_hap_plan; gvl_batch.hap_plan), or NULL
    const int *slot_vidx;   // the slot records' variant indices (gvl_static.slot_vidx): the pipelined kernel's annotated form
    int row_chunks;         // host side: the chunks of chunk_len bases the caller's bound on the longest row makes (pick_chunk)
    int oo_shift;           // 1: out_offsets holds (start, end) PAIRS, row k = out_offsets[2k .. 2k + 1] (gvl_batch.out_bounds: scatter write;
                            // the all-purpose kernel only); 0: consecutive offsets, row k = out_offsets[k .. k + 1]
};


struct LeanArgs {
    const u8 *ref4; const i64 *ref_offsets; const gvl_srec *srec;
    const int *regions; const int *shifts; const i64 *geno_offset_idx; const u8 *to_rc;
    const u8 *alt_alleles;
    const i64 *go_starts; const i64 *go_stops; const gvl_grec *grec; const i64 *alt_offsets;   // slots that overflow their line
    u8 *onehot; u8 *haps; i64 *out_offsets_w;
    u64 *stamps;        // diagnostic builds (-DGVL_DIAG): 16 u64 per row, phase time stamps + the row's class
    i64 n_geno_offsets;
    int n_rows, n_contigs, regions_stride, ploidy_shift, ploidy, L, dbg;
    int chunks;         // LONG launches: 2048-base chunks per row; 1 otherwise
    int sub;            // LONG launches: consecutive chunks of a row one wave takes, one after the other (>= 1)
    int max_row_len;    // RAG launches of recon_lean_rows_kernel: the caller's bound on the longest row (a longer row is reported, gvl_async_error)
    int rows_per_batch;  // recon_lean_rows_kernel (gvl_lean_pipe.inc): rows of every batch of the launch but the last; n_rows = all of them
    int n_batches;
    int front;          // RAG launches of recon_lean_rows_kernel: workgroups at the FRONT of the grid that run the rows beyond PIPE_RAG_MAXT trips, chunks in parallel (0: none)
    int ref_only;       // recon_lean_rows_kernel as gvl_get_reference's kernel: rows = regions, no variants, no shift (regions' third column = the end)
    const i64 *out_offsets;     // recon_lean_kernel<.., LONG, RAGL>: where the batch's rows start and end (ragged long rows)
    const u32 *hplan;           // recon_lean_kernel<.., LONG>: the rows' chunk plans (hap_plan_kernel), or NULL = every chunk-wave walks its row
    const int *slot_vidx;       // recon_lean_rows_kernel<.., ANN>: the variant index of every slot record (gvl_static.slot_vidx)
    const u8 *keep; const i64 *keep_offsets;    // recon_lean_kernel<.., LONG> / hap_plan_kernel: the batch's keep mask (NULL: none) -- a masked variant is
                                                // invisible to the walk (src/reconstruct/mod.rs:86-90)
    int *av; int *ap;           // recon_lean_kernel<.., LONG, .., ANN>: the annotation outputs (annot_v_idxs, annot_ref_pos)
};
static_assert(sizeof(LeanArgs) % 8 == 0, "ReconArgs follows LeanArgs in the kernarg segment");

struct DiffArgs {
    const i64 *geno_offset_idx; i64 n_rows; int ploidy;
    const int *geno_v_idxs; const i64 *go_starts; const i64 *go_stops;
    const int *ilens; const int *v_starts; i64 n_variants;
    const gvl_grec *grec;       // nullable: (pos, ilen) next to the CSR entry, one read instead of three
    const u8 *keep; const i64 *keep_offsets;
    const int *q_starts; const int *q_ends; i64 q_stride;
    int *diffs;
    // fused sizing (ffi/mod.rs:794-811)
    i64 output_length; i64 *lengths;
    // the native loop's ragged batches live in slots of a fixed capacity: a row longer than len_cap (> 0) is
    // cut to it and reported through *async_err (never silently)
    i64 len_cap; int *async_err;
};

struct TrackArgs {
    const i64 *go_starts; const i64 *go_stops; const int *geno_v_idxs; const int *v_starts;
    const int *ilens; i64 n_variants;
    const gvl_grec *grec;       // genotype-inline records (gvl_static.geno_rec; NULL: geno_v_idxs -> v_starts / ilens)
    const int *regions; i64 regions_stride; const int *shifts; const i64 *geno_offset_idx;
    const u8 *keep; const i64 *keep_offsets; const u8 *to_rc; const i64 *out_offsets;
    i64 n_rows; int ploidy; int ploidy_shift; int chunk_len;
    const float *tracks; const i64 *track_offsets;
    double param; i64 strategy; u64 base_seed;
    const u64 *seed_ptr;        // non-NULL: base_seed is read from the device (the native loop's per-batch seeds)
    float *out;
    int dbg;
    const int2 *plan_hdr; const i32x4 *plan_ent;   // non-NULL: the rows' entry tables + per (row, chunk) which of them (track_plan_kernel)
    u64 *stamps;                        // diagnostics (gvl_diag_set_stamps): words 8.. count the chunk-waves that leave the common path
    const i64 *query_seed;              // nullable: local query -> the `query` component of the FlankSample seed (gvl_batch.query_seed)
    int to_shift;                       // 1: track_offsets holds (0, length) PAIRS per query (gvl_tracks_batch's fused path: no scratch track, so no
                                        // prefix sum either); 0: consecutive offsets
};
// A row's plan (track_plan_kernel): the entries of the WHOLE row -- {first value, kind, delta / position, fill length}, in
// output order, at most PLAN_MAXE -- and per chunk {first entry that reaches into it, how many do}; count < 0: not planned,
// the chunk's wave walks the row's variants itself.
constexpr int PLAN_MAXE = 128;
inline i64 track_plan_bytes(i64 n_rows, i64 chunks) {      // headers, 256-byte aligned, then the entry tables
    return ((n_rows * chunks * (i64)sizeof(int2) + 255) & ~255ll) + n_rows * (i64)PLAN_MAXE * (i64)sizeof(i32x4);
}

// ---- internal host interface (defined in the translation unit named) ----------------------------------------------
// gvl_hip.hip
extern thread_local char g_err[512];
extern u64 *g_stamps;
int fail(int code, const char *fmt, const char *what);
int check_launch(const char *what);
int *async_err_word();
int pick_chunk(i64 max_len, int *chunks, int *chunk_len);
int debug_flags();
i64 tune(int key);
int log2_exact(i64 v);
int fill_diff_args(DiffArgs &D, const gvl_static *st, const gvl_batch *bt, const char *who);
// gvl_recon.hip
int launch_recon(const ReconArgs &A, int chunks, int variant, void *stream);
hipError_t pool_alloc(void **p, size_t bytes, hipStream_t s);      // stream-ordered scratch from the library's own pool (free: hipFreeAsync)
// gvl_lean.hip
void fill_lean_args(LeanArgs &A, const ReconArgs &RA, int chunks);     // (memset first)
int launch_lean(const ReconArgs &RA, int chunks, void *stream);
int launch_hap_plan(const ReconArgs &RA, int chunks, u32 *plan, void *stream);
// gvl_lean_pipe.hip
bool lean_pipe_compatible(const ReconArgs *RAs, int n);
int launch_lean_rows(const ReconArgs *RAs, int n, void *stream, int rag_chunks);
// gvl_tracks.hip
int tracks_batch_impl(const gvl_static *st, const gvl_batch *bt, const int64_t *offset_idxs, const gvl_track_set *tracks,
                      int32_t n_tracks, const double *params, int64_t strategy_id, uint64_t base_seed, const u64 *seed_ptr,
                      float *out, int64_t out_track_stride, void *scratch, int64_t scratch_stride, void *stream,
                      const i64 *pre_track_offsets = nullptr, const i64 *pre_out_offsets = nullptr,
                      const int2 *pre_plan_hdr = nullptr, const i32x4 *pre_plan_ent = nullptr);
int launch_track_plan(const TrackArgs &TA, int2 *hdr, i32x4 *ent, int chunks, i64 fixed_len, i64 rows_per_batch_q, void *stream);

}  // namespace gvli
using namespace gvli;
