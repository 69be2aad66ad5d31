// rerank_body.cuh -- the exact re-rank of the keys a matrix-core filter kept, with the exactness certificate (device code shared by the
// stand-alone knn_mfma_rerank_kernel and by the re-rank role of launch B, frame_b_kernel), plus the error bounds of the three filters.
// Included by knn_mfma_kernels.hip inside namespace lcd { namespace { ... } }, behind the filter and the frame-tail bodies.

// |bf16x3 filter score - reference distance| <= eps, u = 2^-24:
//   split: bf16 keeps 8 significant bits (unit roundoff 2^-8): x = hi + lo + d with |lo| <= 2^-8 |x|, |d| <= 2^-8 |lo| <= 2^-16 |x|;
//          the neglected ql.vl and the two d terms cost <= 3 * 2^-16 |q||v| (1 + 2^-7) on q.v, twice that on the score
//          -> 3.1 * 2^-16 (|v|^2 + |q|^2)   (tests/test_bf16_split_bound.py emulates the split on the CPU: adversarial inputs reach
//          a third of it)
//   accumulation: 2 + 3 dim products summed in fp32 by the matrix pipe; each addition is charged 2u (round-to-nearest or
//          truncation) of the running magnitude <= |v|^2 + |q|^2 + 2 * 3 |q||v| <= 4 (|v|^2 + |q|^2)  -> (3 dim + 4) * 2u * 4 (..)
//   norms (dim-term FMA chains) and the reference's own rounding, as in eps_for()                     -> (dim + 2 (dim/4 + 6)) u (..)
// a quarter more is added for slack; the measured worst case is reported by the tests (knn_max_err_ratio).
__device__ __forceinline__ float eps_bf16(int dim, float qn, float vn_max) {
    const float u = 5.9604645e-8f;
    return (3.1f * 1.5258789e-5f + ((3.0f * (float)dim + 4.0f) * 8.0f + 1.5f * (float)dim + 12.0f) * u) * 1.25f * (qn + vn_max);
}
// |fp16 one-product filter score - reference distance| <= eps: both operands rounded to half (u16 = 2^-11, relative, inside half's normal
// range): |q16.v16 - q.v| <= (2 u16 + u16^2) |q||v|, i.e. (2 u16 + u16^2)(|q|^2 + |v|^2) on the score -2 q.v (tests/test_fp16_split_bound.py);
// components below half's normal range (2^-14) are rounded with an ABSOLUTE error <= 2^-25 each: 2 * dim * 2^-25 (|q| + |v|) more on the
// score, charged with |x| <= 1 + |x|^2; the accumulation (dim products in fp32 by the matrix pipe) and norm terms as in eps_bf16.
__device__ __forceinline__ float eps_f16(int dim, float qn, float vn_max) {
    const float u = 5.9604645e-8f, u16 = 4.8828125e-4f;
    return ((2.0f * u16 + u16 * u16) + (((float)dim + 4.0f) * 8.0f + 1.5f * (float)dim + 12.0f) * u) * 1.25f * (qn + vn_max) +
           2.0f * (float)dim * 2.9802322e-8f * (2.0f + qn + vn_max);
}

// ------------------------------------------------------------------------------------------------ re-rank + certificate
// |filter score - reference distance| <= eps: both are fp32 evaluations of the same real number d = |v - q|^2 <= 2 (|v|^2 + |q|^2).
// With u = 2^-24 and gamma_n ~ n u:
//   filter: a chain of dim + 2 FMAs over terms whose magnitudes sum to <= 2 (|v|^2 + |q|^2)        -> 2 (dim + 2) u (|v|^2 + |q|^2)
//           the two norms are themselves dim-term FMA chains                                          ->       dim u (|v|^2 + |q|^2)
//   reference (dist.h:150-177): every term (v_k - q_k)^2 carries 3 roundings, then dim/4 + 3 additions
//           of non-negative numbers                                                                   -> 2 (dim/4 + 6) u (|v|^2 + |q|^2)
// total (3.5 dim + 16) u (|v|^2 + |q|^2); a quarter more is added for slack.  |v|^2 is replaced by the vocabulary maximum.
__device__ __forceinline__ float eps_for(int dim, float qn, float vn_max) {
    return (3.5f * (float)dim + 16.0f) * 5.9604645e-8f * 1.25f * (qn + vn_max);
}

// One workgroup per query (the kernel is a chain of dependent memory round trips: the more lanes share them, the shorter).
// Pass 1 finds tau = the second smallest filter score among the kept keys; a kept row whose score exceeds
// tau (1 + 2^-15) + 2 eps is strictly farther than the two rows that define tau (|score - distance| <= eps, keys are truncated by
// < 2^-16 relative), so only the few keys at or below that threshold are re-computed exactly in pass 2 -- each by 16 lanes:
// lane i of the group holds the term of floats [4i, 4i + 4) (one coalesced 256-byte row read) and the sixteen terms are added in
// the reference's order.  Nothing is dropped at this stage (more than RR_MAX_CAND keys under the threshold -- a cluster of
// near-identical rows -- sends the query to the exact scan): the bound on dropped rows comes from the filter alone.
// KEEP keys per (row block, query); LAST_KEY_BOUNDS: the block's last kept key also bounds what its merge dropped (f32 filter);
// BF16: the keys come from the bf16x3 filter (eps_bf16).  fail_count[2] collects max |score - distance| / eps (diagnostics).
constexpr int RR_MAX_CAND = 128;
#ifdef LCD_B_TIMING   // timing experiment only: phases of the re-rank workgroups of launch B (100 MHz), without extra barriers
__device__ unsigned long long g_rr_timing[8 * 512];
#define RR_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x < 512) g_rr_timing[8 * blockIdx.x + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
// the tail behind the barrier, per workgroup (tools/launch_b_tail.py): [0] bit row and list stored, [1] candidate rows, [2] list entries, [3] XCD.
// LCD_RR_ACKSTAMP: the stamps behind stores (7, tail 0, the end of the workgroup) first wait for every request of their wave to be acknowledged --
// what a phase COSTS in round trips, where the plain stamps say when its stores were issued
__device__ unsigned long long g_rr_tail[4 * 512];
#define RR_TAIL(i, v) do { if (threadIdx.x == 0 && blockIdx.x < 512) g_rr_tail[4 * blockIdx.x + (i)] = (v); } while (0)
#define RR_XCD() ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (3 << 11)))   /* hardware register XCC_ID, bits [3:0] */
#ifdef LCD_RR_ACKSTAMP
#define RR_ACK() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define RR_ACK() do { } while (0)
#endif
#else
#define RR_STAMP(i) do { } while (0)
#define RR_TAIL(i, v) do { } while (0)
#define RR_XCD() 0ull
#define RR_ACK() do { } while (0)
#endif
// the reference's term of four floats (dist.h:158-166): ((d0 d0 + d1 d1) + d2 d2) + d3 d3, every difference, product and sum rounded on its own
__device__ __forceinline__ float l2_term4(const float4& v, const float4& q) {
    const float d0 = __fsub_rn(v.x, q.x), d1 = __fsub_rn(v.y, q.y), d2 = __fsub_rn(v.z, q.z), d3 = __fsub_rn(v.w, q.w);
    float t = __fmul_rn(d0, d0);
    t = __fadd_rn(t, __fmul_rn(d1, d1));
    t = __fadd_rn(t, __fmul_rn(d2, d2));
    return __fadd_rn(t, __fmul_rn(d3, d3));
}

// The staging area of the pending rows (64 floats each).  Slot (row r, position s) holds the row's 16-byte chunk s ^ (r & 15): sixteen consecutive
// lanes that read the same chunk of sixteen consecutive rows touch sixteen different positions (no bank conflict).  The rows come in by LDS-DMA,
// which writes linearly (wave-uniform base + 16 B x lane), so the swizzle is applied to the SOURCE address:
//   stage_four_rows: instruction i of the area, issued by one wave, brings rows 4 i .. 4 i + 3 = 1 KB of LDS (lane ln: position ln & 15 of row
//                    4 i + (ln >> 4)); row_src(rl) is the address of staged row rl < n_rows (the rows of a partial last group repeat the last row)
//   staged_chunk:    where chunk c of staged row r lies
template <class RowSrc>
__device__ __forceinline__ void stage_four_rows(float* stage, int i, int ln, int n_rows, RowSrc row_src) {
    const int r = i * 4 + (ln >> 4);
    const float* src = row_src(min(r, n_rows - 1));
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + ((ln & 15) ^ (r & 15)) * 4),
                                     (__attribute__((address_space(3))) void*)(stage + (size_t)i * 256), 16, 0, 0);
}
__device__ __forceinline__ const float4* staged_chunk(const float* stage, int r, int c) {
    return reinterpret_cast<const float4*>(stage + (size_t)r * 64) + (c ^ (r & 15));
}

// HALVES = 2: a workgroup of 2 x MF_BLOCK threads re-ranks TWO queries (qi_first, qi_first + 1), one per half -- launch B of a
// pipelined frame runs with 512-thread workgroups because its scoring half needs eight waves per bucket (a 4-wave scoring workgroup
// takes twice as long), and a re-rank workgroup that used only half of its threads idled the other.  The halves share nothing but the
// barriers (every barrier of the body is reached by all threads: the conditions around them are launch-uniform).
// The phases: rows-only exit | up-front requests | pass 1 (tau, bound) | staging of the pending rows | pass 2 (candidates) | exact distances |
// pending scan | top-2 and winner slots | results and certificate | candidate bits | row writes and mirror.
// What the filter kept for the re-rank, by the filter's kind -- the body's BF16 flag picks the type, so a caller cannot fill the other form:
//   KeptKeys<true>   `records`, one StripRecord per (row block, query) of a bf16 / fp16 filter (bf16_filter_body.cuh), whose blocks are
//                    tiles_per_block tiles each;
//   KeptKeys<false>  the f32 filter's query-major arrays, keys [q][n_blocks][KEEP] and lmin [q][n_blocks].
template <bool BF16> struct KeptKeys;
template <> struct KeptKeys<true> { const StripRecord* records; int tiles_per_block; };
template <> struct KeptKeys<false> { const uint64_t* keys; const uint32_t* lmin; };
template <int DIM, int KEEP, bool LAST_KEY_BOUNDS, bool BF16, int HALVES = 1>
__device__ __forceinline__ void knn_mfma_rerank_body(int qi_first, const KeptKeys<BF16>& kk, int n_blocks, int nq,
                                                     const float* __restrict__ vocab, const float* __restrict__ queries,
                                                     const int32_t* __restrict__ row_id,
                                                     const uint32_t* __restrict__ norm_max_bits,
                                                     int32_t* __restrict__ out_row, int32_t* __restrict__ out_word,
                                                     float* __restrict__ out_dist, int32_t* __restrict__ fail_list,
                                                     int32_t* __restrict__ fail_count, const CandBits& cb,
                                                     const int32_t* __restrict__ pend_lo = nullptr, const int32_t* __restrict__ pend_hi = nullptr,
                                                     int pend_cap = 0x7fffffff /* rows the filter's launch plan covered */,
                                                     float* stage = nullptr, int stage_rows = 0 /* LDS staging area of the pending rows (256 B each,
                                                     a multiple of 4), shared by the halves of the workgroup */,
                                                     int f16 = 0 /* the keys come from the one-product fp16 filter (eps_f16) */,
                                                     const float* __restrict__ pend_desc = nullptr, const uint32_t* __restrict__ pend_list = nullptr,
                                                     int32_t pend_first_id = 0
                                                     /* rows at or beyond pend_lo[0] are not vocabulary rows yet (a deferred append writes them in this
                                                        very launch): row pend_lo[0] + j is descriptor pend_list[j] of pend_desc, word pend_first_id + j */
                                                     , const float* __restrict__ cross = nullptr, int cross_ld = 0
                                                     /* cross[qi * cross_ld + c] = |query qi - descriptor c of pend_desc|^2, from the cross-frame tiles of
                                                        launch A of this pair (selfdist_tile): the pending rows' distances are read, not computed; NULL: the
                                                        rows are staged and their distances computed here */
                                // The re-rank workgroups WRITE the rows of the deferred append from the copy they have staged anyway (round 5: the
                                // default since it passed the GPU suite; launch B 15.3 -> 13.8 us at the headline, profiles/r05_first_call.txt);
                                // workgroup wr_index of wr_n
                                                     , const AppendRowsArgs& wr = AppendRowsArgs(), bool wr_on = false, int wr_index = 0, int wr_n = 1
                                // rows_only (round 6, PipeOpts::row_writer_wgs): this workgroup re-ranks nothing -- it is one of wr_n extra workgroups of
                                // the re-rank ROLE that only write the appended rows (wr_index, wr_index + wr_n, ...), so that no re-rank workgroup has
                                // the row stores at the end of its chain (the workgroups that wrote a row ended 3-4 us after those that did not) and
                                // the kernel gets no third branch (whose register demand made the scoring branch spill)
                                                     , bool rows_only = false
                                // shadow scores (round 6): sh_x[qi * sh_ld + j] is the filter's score of this query against descriptor j of the frame before
                                // (sh_q of them; shadow_scores_body of launch A).  Descriptor j is a row of the vocabulary iff bit j of sh_mask is set (the
                                // final new-word mask of that frame's decision loop, mw words, followed by its mw + 1 word prefix sums): row n_lo0 + rank(j),
                                // word pend_first_id + rank(j), read from pend_desc.  The words whose score is at or below the threshold join the candidates
                                // as keys of ONE row (SHADOW_ROW_BASE + j) and are evaluated exactly in the same round trip as the others; a word above the
                                // threshold cannot be among the two nearest, by the argument that covers every kept key above it.  The rows [n_lo0, p_hi)
                                // then need no scan of their own (and are written by the rows_only workgroups).
                                                     , const uint32_t* __restrict__ sh_mask = nullptr, int sh_q = 0, const float* __restrict__ sh_x = nullptr, int sh_ld = 0
                                                     ) {
    static_assert(DIM == 64, "16 lanes x 4 floats per candidate row");
    constexpr int NT = HALVES * MF_BLOCK;                              // threads of the workgroup
    // (both counters through the scalar cache, requested together: as two vector loads the compiler made each uniform right behind its request --
    // two round trips in a row at the head of every re-rank workgroup, round 6's ISA)
    // err_seen: fail_count[2], the running maximum of the error ratio, as some earlier moment saw it (the scalar cache may hold an older line).  It only
    // ever rises, so a stale value is never above the current one: a query whose ratio does not exceed it has nothing to add, and only the others
    // issue the atomic -- a handful in the first frames of a stream, then almost none (it was one device-scope atomic per query, ~500 per launch on
    // one address, in front of the result stores in the one in-order counter)
    int n_lo0 = 0, p_hi_ld = 0;
    uint32_t err_seen = 0u;
    if (pend_lo && pend_hi)
        asm volatile("s_load_dword %0, %3, 0x0\n\ts_load_dword %1, %4, 0x0\n\ts_load_dword %2, %5, 0x8\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(n_lo0), "=&s"(p_hi_ld), "=&s"(err_seen) : "s"(pend_lo), "s"(pend_hi), "s"(fail_count) : "memory");
    else {
        if (pend_lo) n_lo0 = pend_lo[0];
        if (pend_hi) p_hi_ld = pend_hi[0];
        asm volatile("s_load_dword %0, %1, 0x8\n\ts_waitcnt lgkmcnt(0)" : "=s"(err_seen) : "s"(fail_count) : "memory");
    }
    const int p_lo = pend_lo ? min(n_lo0, pend_cap) : 0, p_hi = p_hi_ld;
    const int32_t pend_id0 = pend_first_id > 0 ? pend_first_id : n_lo0 - pend_first_id;   // word id of the first pending row
    // with shadow rows the pending scan only has to cover vocabulary rows the filter's plan did not reach ([p_lo, n_lo0): rare)
    const int p_hi_s = sh_q > 0 ? min(p_hi, n_lo0) : p_hi;
    // the pinned row-count mirror of the frame whose rows this launch writes, when its decision loop left it to this launch (AppendArgs::mirror_later):
    // one thread of the launch, at the END of its workgroup's body (a store to host memory in front of a load would hold that load for its acknowledgement)
    auto store_mirror = [&]() {
        const AppendArgs& ap = wr.ap;
        if (ap.mirror_later && ap.host_mirror && wr_on && wr_index == 0 && threadIdx.x == 0)
            __hip_atomic_store(ap.host_mirror, ((unsigned long long)ap.tag << 32) | (unsigned long long)(uint32_t)p_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    // a writer workgroup without rows to write leaves here, in front of every request (a request nobody waits for would be waited for at the mirror's store)
    if (rows_only && (!wr_on || stage == nullptr || stage_rows < 4 || pend_list == nullptr || p_hi - n_lo0 <= wr_index)) { store_mirror(); return; }
    __shared__ uint32_t s_plist[NT];                                   // the first entries of pend_list (one per thread: read with the keys)
    uint32_t plreg = 0u, shreg = 0u;                                   // (requested behind the keys; the writers request theirs below)
    auto plist_at = [&](int j) -> uint32_t { return j < NT ? s_plist[j] : pend_list[j]; };
    constexpr int SH_MW_MAX = 128;                                     // mask words of a frame of 4 096 descriptors
    __shared__ uint32_t s_shmask[2 * SH_MW_MAX + 1];
    const int sh_mw = sh_q > 0 ? (sh_q + 63) / 64 * 2 : 0;
    auto sh_isword = [&](uint32_t j) -> bool { return (s_shmask[j >> 5] >> (j & 31)) & 1u; };
    auto sh_rank = [&](uint32_t j) -> int { return (int)(s_shmask[sh_mw + (j >> 5)] + (uint32_t)__popc(s_shmask[j >> 5] & ((1u << (j & 31)) - 1u))); };
    const int hf = HALVES == 2 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / MF_BLOCK) : 0;   // (uniform over the wave: the query index and all that follows from it stay scalar)
    const int tid = HALVES == 2 ? (int)threadIdx.x % MF_BLOCK : (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // The pending rows are the same for every query: with a staging area they come in by LDS-DMA -- no registers, requested in front of pass 2,
    // a whole chunk in one round trip that runs under the two passes -- instead of four rows per 16-lane group and trip
    // (three dependent round trips for the ~150 words a frame creates: +7 us on launch B, measured).
    auto stage_chunk = [&](int first, int n_chunk) {
        const int wv = (int)threadIdx.x >> 6, ln = (int)threadIdx.x & 63;       // (wave of the WORKGROUP: both halves stage rows together)
        // every re-rank workgroup of the launch wants the SAME rows at the same moment: each starts at another row (rotation by workgroup
        // index), so that at any time the requests spread over all the L2 channels instead of queueing at one
        const int n_inst = (n_chunk + 3) / 4;
        const int rot = (int)(((unsigned)blockIdx.x * 13u) % (unsigned)n_inst);
        auto issue = [&](auto list_at) {
            for (int i0 = wv; i0 < n_inst; i0 += HALVES * MF_WAVES) {
                const int i = i0 + rot < n_inst ? i0 + rot : i0 + rot - n_inst;
                stage_four_rows(stage, i, ln, n_chunk, [&](int rl) -> const float* {
                    const int r = first + rl;                           // a row that is being written in this launch: its descriptor
                    return (pend_list && r >= n_lo0) ? pend_desc + (size_t)list_at(r - n_lo0) * DIM : vocab + (size_t)r * DIM;
                });
            }
        };
        // every list entry the chunk can need lies in s_plist: the common case gets a loop of its own without any read from memory.  (The other
        // case -- a frame that created more than NT words -- reads the list inside the issue loop, and a read there makes every trip wait for the
        // requests of the trip before it (one in-order counter): five serial round trips instead of one, 2.6 us on the ~150 rows a frame creates.)
        if (!pend_list || first + n_chunk - n_lo0 <= NT) issue([&](int j) -> uint32_t { return s_plist[j]; });
        else issue(plist_at);
    };
    // With the cross-frame matrix the pending rows need no staging: row n_lo0 + j is descriptor pend_list[j] of the frame before, and the
    // query's distance to it is cross[qi][pend_list[j]] -- in the reference's arithmetic, computed by launch A.  Each workgroup stages only the
    // rows it WRITES (row wr_index + m wr_n at place m), and the distances are gathered into the staging area by 4-byte LDS-DMA (no registers):
    // half hf's value j at xd[hf * XD_MAX + j].  Not when rows of the vocabulary itself are pending (the plan covered fewer rows than exist).
    constexpr int XD_MAX = 2048, XD_OWN = 32;                           // pending rows / rows of its own a workgroup can take this way (40 KB of LDS)
    const int n_own = (wr_on && p_hi - n_lo0 > wr_index) ? (p_hi - n_lo0 - wr_index + wr_n - 1) / wr_n : 0;
    const bool use_cross = sh_q == 0 && cross != nullptr && pend_list != nullptr && stage != nullptr && stage_rows >= XD_OWN + HALVES * XD_MAX / DIM && p_hi > p_lo &&
                           p_lo == n_lo0 && p_hi - p_lo <= XD_MAX && n_own <= XD_OWN;
    float* const xd = stage + XD_OWN * DIM;
    const bool staged = stage != nullptr && stage_rows >= 4 && p_hi_s > p_lo && !use_cross;
    // rows [n_lo0, p_hi) ARE the rows of the deferred append: workgroup wr_index of wr_n writes rows wr_index, wr_index + wr_n, ... (16 lanes per row)
    // from its staging area -- no workgroups of their own, no third branch in the kernel (whose presence makes the scoring branch spill,
    // DESIGN.md 7a).  Stores only, at the END of the body: a read behind them would wait for them.
    // The staging area holds the n_chunk rows from vocabulary row c0 on, or (own) this workgroup's rows only, staged row m being its m-th row.
    auto write_rows = [&](int c0, int n_chunk, bool own = false) {
        const AppendArgs& ap = wr.ap;
        const int n_new = p_hi - n_lo0, c16 = (int)threadIdx.x & 15;
        float nmax = 0.0f;
        for (int j = wr_index + wr_n * ((int)threadIdx.x >> 4), m = (int)threadIdx.x >> 4; j < n_new; j += wr_n * (NT / 16), m += NT / 16) {
            const int rl = own ? m : n_lo0 + j - c0;                   // the row's place in the staged chunk (uniform over its 16 lanes)
            if (rl < 0 || rl >= n_chunk) continue;
            const int32_t key = (c16 == 0 && wr.new_ws.n > 0) ? ws_runs_at_dev(wr.new_ws, j) : -1;      // (looked up in front of the row's stores)
            const uint4 x = *reinterpret_cast<const uint4*>(staged_chunk(stage, rl, c16));
            append_write_row(ap, (size_t)n_lo0 + (size_t)j, c16, x, nmax);
            if (c16 == 0) {
                const size_t row = (size_t)n_lo0 + (size_t)j;
                ap.row_id[row] = ap.first_id > 0 ? ap.first_id + j : (int32_t)row - ap.first_id;    // (first_id <= 0: the id follows the ROW, AppendArgs)
                ap.row_wslot[row] = key;
                if (key >= 0 && ap.wrow) ap.wrow[key] = (uint32_t)row + 1u;
            }
        }
        append_norm_max(ap, nmax);
    };

    // ---- rows-only exit: a writer workgroup of the re-rank role stages its rows (wr_index + wr_n m, m < n_mine) and writes them
    if (rows_only) {                                                 // (uniform over the workgroup)
        const int n_new = p_hi - n_lo0;
        const uint32_t nm_seen = running_max_seen(wr.ap.norm_max_bits);   // (frame_tail_body.cuh: sixteen writers x eight waves would each raise it)
        s_plist[threadIdx.x] = pend_list[threadIdx.x];
        lds_barrier();
        const int wv = (int)threadIdx.x >> 6, ln = (int)threadIdx.x & 63;       // (wave of the WORKGROUP: both halves stage rows together)
        const int n_mine = (n_new - wr_index + wr_n - 1) / wr_n;
        const int cap = stage_rows & ~3;
        for (int m0 = 0; m0 < n_mine; m0 += cap) {                     // (one chunk unless a frame creates more than wr_n x 160 words)
            const int n_chunk = min(cap, n_mine - m0);
            if (m0 > 0) __syncthreads();
            for (int i = wv; i * 4 < n_chunk; i += HALVES * MF_WAVES)
                stage_four_rows(stage, i, ln, n_chunk, [&](int rl) -> const float* { return pend_desc + (size_t)plist_at(wr_index + wr_n * (m0 + rl)) * DIM; });
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (m0 == 0) { RR_STAMP(6); RR_TAIL(3, RR_XCD()); }
            {   // write_rows(own = true) over this chunk, staged row m being new word wr_index + wr_n (m0 + m).  A copy, not a call: as a call with a
                // first-row argument it costs frame_b_kernel<false> two more s_waitcnt (profiles/refactor_rerank_body_isa.txt)
                const AppendArgs& ap = wr.ap;
                const int c16 = (int)threadIdx.x & 15;
                float nmax = 0.0f;
                for (int m = (int)threadIdx.x >> 4; m < n_chunk; m += NT / 16) {
                    const int j = wr_index + wr_n * (m0 + m);
                    const int32_t key = (c16 == 0 && wr.new_ws.n > 0) ? ws_runs_at_dev(wr.new_ws, j) : -1;
                    const uint4 x = *reinterpret_cast<const uint4*>(staged_chunk(stage, m, c16));
                    append_write_row(ap, (size_t)n_lo0 + (size_t)j, c16, x, nmax);
                    if (c16 == 0) {
                        const size_t row = (size_t)n_lo0 + (size_t)j;
                        ap.row_id[row] = ap.first_id > 0 ? ap.first_id + j : (int32_t)row - ap.first_id;
                        ap.row_wslot[row] = key;
                        if (key >= 0 && ap.wrow) ap.wrow[key] = (uint32_t)row + 1u;
                    }
                }
                append_norm_max(ap, nmax, nm_seen);
            }
        }
        store_mirror();
        RR_ACK();
        RR_STAMP(7);
        return;
    }
    const bool valid = qi_first + hf < nq;                           // the odd query out: its half walks the last query again, writes nothing
    const int qi = valid ? qi_first + hf : nq - 1;
    __shared__ float s_thr_all[HALVES];
    float& s_thr = s_thr_all[hf];
    const int n_keys = n_blocks * KEEP;
    constexpr int GS = BF16 ? 4 : 1;                                   // rows a key stands for (see the exact phase)
    constexpr int RR_KEYS = RR_MAX_CAND / GS;                          // keys under the threshold a query may have before it goes to the exact redo
    // The bf16 / fp16 filters leave ONE 16-byte record per (block, query), block-major (StripRecord: both kept keys and the bound, one request);
    // the f32 filter query-major arrays: key c of the query is block c / KEEP, entry c % KEEP
    static_assert(!BF16 || KEEP == BF_KEEP, "a StripRecord holds BF_KEEP keys");
    const int qpad_t = (nq + 63) / 64 * 64;
    constexpr uint32_t INF = 0x7f800000u;
    // (each accessor exists for its own form only: the other form's members are not there to be read)
    auto rec_at = [&](int b) -> uint4 {
        if constexpr (BF16) return *reinterpret_cast<const uint4*>(kk.records + (size_t)b * qpad_t + qi); else return make_uint4(0u, 0u, 0u, 0u);
    };
    auto rec_tile0 = [&](int b) -> int { if constexpr (BF16) return b * kk.tiles_per_block; else return 0; };   // the first tile of block b
    auto key_at = [&](int c) -> uint64_t { if constexpr (!BF16) return kk.keys[(size_t)qi * n_keys + c]; else return KEY_NONE; };
    auto bound_at = [&](int b) -> uint32_t { if constexpr (!BF16) return kk.lmin[(size_t)qi * n_blocks + b]; else return INF; };
    __shared__ uint32_t s_a0_all[HALVES][MF_WAVES], s_a1_all[HALVES][MF_WAVES], s_bound_all[HALVES][MF_WAVES];
    __shared__ int s_ncand_all[HALVES];
    __shared__ uint64_t s_cand_all[HALVES][RR_MAX_CAND], s_exact_all[HALVES][RR_MAX_CAND];
    __shared__ int32_t s_word_all[HALVES][RR_MAX_CAND];
    __shared__ float s_err_all[HALVES][MF_WAVES];
    __shared__ uint64_t s_pend_all[HALVES][MF_WAVES][2];
    uint32_t (&s_a0)[MF_WAVES] = s_a0_all[hf]; uint32_t (&s_a1)[MF_WAVES] = s_a1_all[hf]; uint32_t (&s_bound)[MF_WAVES] = s_bound_all[hf];
    int& s_ncand = s_ncand_all[hf];
    uint64_t (&s_cand)[RR_MAX_CAND] = s_cand_all[hf]; uint64_t (&s_exact)[RR_MAX_CAND] = s_exact_all[hf];
    int32_t (&s_word)[RR_MAX_CAND] = s_word_all[hf];
    float (&s_err)[MF_WAVES] = s_err_all[hf];
    uint64_t (&s_pend)[MF_WAVES][2] = s_pend_all[hf];
    // the query slice of every lane (chunk lane & 15) is needed up to the last exact distance: it lives in LDS, not in four registers held across the whole body
    __shared__ float4 s_q_all[HALVES][16];
    const float4* const s_q = s_q_all[hf];

    // ---- up-front requests.  Everything that does not depend on other loads is requested here (the kernel is a chain of round trips): the
    // thread's first two records (f32 filter: its first three keys and first bound), the query slice, the vocabulary norm bound, -- for the candidate bits -- the
    // thread's two entries of the query's row of the same-frame distance matrix, the shadow scores and, LAST, the thread's list and mask entries:
    // requested in front of the keys (where they used to be) they are waited for before the first key's address is formed -- a round trip of
    // their own at the head of every re-rank workgroup.
    // Register budget (frame_b_kernel<false>: 80, no scratch -- tests/test_pipeline_scratch.py): the query slice goes to LDS as soon as its norm
    // is taken, the waves' bounds stay in LDS until the certificate, and the half / query index is scalar.
    RR_STAMP(0);
    // BF16: the thread's first two records (219 strips at the headline: one request per thread, none for the last 37), nothing else of the filter's
    const uint4 rec_none = make_uint4(REC_KEY_NONE, REC_KEY_NONE, INF, 0u);
    uint4 rreg0 = rec_none, rreg1 = rec_none;
    uint64_t kreg0 = KEY_NONE, kreg1 = KEY_NONE, kreg2 = KEY_NONE;
    uint32_t breg0 = INF;
    if constexpr (BF16) {
        // (no condition on the requests: a load under a condition gets a wait of its own inside its branch -- the ISA of the first version of
        // this block had one behind each record, two round trips in front of the query's.  A thread without a block asks for the last block's
        // record, which its neighbours fetch anyway, and drops it in front of pass 1; the buffer holds a block's records even when there is none)
        const int b_last = max(n_blocks - 1, 0);
        rreg0 = rec_at(min(tid, b_last));
        rreg1 = rec_at(min(tid + MF_BLOCK, b_last));
    } else {
        if (tid < n_keys) kreg0 = key_at(tid);
        if (tid + MF_BLOCK < n_keys) kreg1 = key_at(tid + MF_BLOCK);
        if (tid + 2 * MF_BLOCK < n_keys) kreg2 = key_at(tid + 2 * MF_BLOCK);
        if (tid < n_blocks) breg0 = bound_at(tid);
    }
    const float4 q4 = reinterpret_cast<const float4*>(queries + (size_t)qi * DIM)[lane & 15];
    const float vn_max = __uint_as_float(norm_max_bits[0]);
    float dreg0 = __int_as_float(0x7f800000), dreg1 = __int_as_float(0x7f800000);
    if (cb.bits) {
        if (tid < cb.nq) dreg0 = cb.selfdist[(size_t)qi * cb.ld + tid];
        if (tid + MF_BLOCK < cb.nq) dreg1 = cb.selfdist[(size_t)qi * cb.ld + tid + MF_BLOCK];
    }
    float2 xsh = make_float2(__int_as_float(0x7f800000), __int_as_float(0x7f800000));   // the query's scores against descriptors 2 tid, 2 tid + 1 of the frame before
    if (sh_q > 0 && 2 * tid < sh_ld) xsh = *reinterpret_cast<const float2*>(sh_x + (size_t)qi * sh_ld + 2 * tid);
    if (pend_list) plreg = pend_list[threadIdx.x];                     // (the list buffer holds at least NT entries)
    if (sh_q > 0 && (int)threadIdx.x < 2 * sh_mw + 1) shreg = sh_mask[threadIdx.x];
    float qn = fmaf(q4.w, q4.w, fmaf(q4.z, q4.z, fmaf(q4.y, q4.y, q4.x * q4.x)));
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) qn += __shfl_xor(qn, m, 64);

    // ---- pass 1: tau and the bound on dropped rows
    uint32_t a0 = INF, a1 = INF, bound = breg0;
    auto see_score = [&](uint32_t sc) {
        const uint32_t h = max(a0, sc);
        a0 = min(a0, sc);
        a1 = min(a1, h);
    };
    auto see = [&](uint64_t key, int c) {
        const uint32_t sc = min((uint32_t)(key >> 32), INF);                // KEY_NONE -> +inf
        if (LAST_KEY_BOUNDS && (c % KEEP) == KEEP - 1) bound = min(bound, sc);   // rows the block merge dropped are no better than its last key
        see_score(sc);
    };
    auto see_record = [&](const uint4& r) { see_score(record_score(r.x)); see_score(record_score(r.y)); bound = min(bound, r.z); };
    if constexpr (BF16) {
        if (tid >= n_blocks) rreg0 = rec_none;                             // (a thread without a block: see the requests)
        if (tid + MF_BLOCK >= n_blocks) rreg1 = rec_none;
        see_record(rreg0);
        see_record(rreg1);
        for (int b = tid + 2 * MF_BLOCK; b < n_blocks; b += MF_BLOCK) see_record(rec_at(b));
    } else {
        see(kreg0, tid);
        see(kreg1, tid + MF_BLOCK);
        see(kreg2, tid + 2 * MF_BLOCK);
        for (int c = tid + 3 * MF_BLOCK; c < n_keys; c += MF_BLOCK) see(key_at(c), c);
        for (int c = tid + MF_BLOCK; c < n_blocks; c += MF_BLOCK) bound = min(bound, bound_at(c));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o0 = (uint32_t)__shfl_xor((int)a0, m, 64), o1 = (uint32_t)__shfl_xor((int)a1, m, 64);
        a1 = min(max(a0, o0), min(a1, o1));
        a0 = min(a0, o0);
        bound = min(bound, (uint32_t)__shfl_xor((int)bound, m, 64));
    }
    if (lane == 0) { s_a0[wave] = a0; s_a1[wave] = a1; s_bound[wave] = bound; }
    if (tid == 0) s_ncand = 0;

    // ---- staging of the pending rows: requested here -- behind the keys, which have arrived, and in front of pass 2's row reads, whose round
    // trip they share (a request in front of the keys would make the first use of a key wait for the whole chunk: the counter is in-order)
    // (measured in round 5, profiles/r05_ab_notes.txt 8: requested in FRONT of the keys instead, the driver's 20 steps take 0.0392-0.0401 ms
    // per frame against 0.0384-0.0390)
    if (pend_list || sh_q > 0) {
        s_plist[threadIdx.x] = plreg;
        if ((int)threadIdx.x < 2 * sh_mw + 1) s_shmask[threadIdx.x] = shreg;
        lds_barrier();
    }
    if (staged) stage_chunk(p_lo, min(stage_rows, p_hi_s - p_lo));
    if (use_cross) {
        const int wv = (int)threadIdx.x >> 6, ln = (int)threadIdx.x & 63;       // (wave of the WORKGROUP: both halves stage rows together)
        for (int i = wv; i * 4 < n_own; i += HALVES * MF_WAVES)        // the rows this workgroup writes
            stage_four_rows(stage, i, ln, n_own, [&](int rl) -> const float* { return pend_desc + (size_t)plist_at(wr_index + wr_n * rl) * DIM; });
        const int n_pend = p_hi - p_lo;
        const float* crow = cross + (size_t)qi * cross_ld;
        for (int j0 = 0; j0 < n_pend; j0 += MF_BLOCK) {                // 64 values per instruction, lane l's at the instruction's base + 4 l
            const float* src = crow + plist_at(min(j0 + tid, n_pend - 1));
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(xd + hf * XD_MAX + j0 + wave * 64), 4, 0, 0);
        }
    }
    if (lane < 16 && wave == 0) s_q_all[hf][lane] = q4;                // the query, for every lane
    lds_barrier();                                                     // (LDS traffic only: __syncthreads() would also wait for the rows just requested)
    RR_STAMP(1);
    a0 = s_a0[0]; a1 = s_a1[0];                                        // (the waves' bounds stay in LDS until the certificate reads them)
#pragma unroll
    for (int wi = 1; wi < MF_WAVES; ++wi) {
        const uint32_t o0 = s_a0[wi], o1 = s_a1[wi];
        a1 = min(max(a0, o0), min(a1, o1));
        a0 = min(a0, o0);
    }
    const float eps = BF16 ? (f16 ? eps_f16(DIM, qn, vn_max) : eps_bf16(DIM, qn, vn_max)) : eps_for(DIM, qn, vn_max);
    const float tau = __uint_as_float(a1);
    const float thr = tau + (2.0f * eps + tau * 3.0517578e-5f);               // +inf when fewer than two finite keys exist

    // ---- pass 2: the keys at or below the threshold (+inf: tombstone / padding row) ...
    auto take = [&](uint64_t key) {
        const uint32_t sc = (uint32_t)(key >> 32);
        if (key != KEY_NONE && sc < INF && __uint_as_float(sc) <= thr) {
            const int slot = atomicAdd(&s_ncand, 1);
            if (slot < RR_KEYS) s_cand[slot] = key;
        }
    };
    // (a record's keys are widened HERE, and only those under the threshold: record_widen, the block's first tile from its index)
    auto take_record = [&](const uint4& r, int b) {
        const uint32_t rk[BF_KEEP] = {r.x, r.y};
#pragma unroll
        for (int e = 0; e < BF_KEEP; ++e) {
            const uint32_t sc = record_score(rk[e]);                           // (KEY_NONE -> +inf)
            if (sc < INF && __uint_as_float(sc) <= thr) {
                const int slot = atomicAdd(&s_ncand, 1);
                if (slot < RR_KEYS) s_cand[slot] = record_widen(rk[e], rec_tile0(b));
            }
        }
    };
    if constexpr (BF16) {
        take_record(rreg0, tid);
        take_record(rreg1, tid + MF_BLOCK);
        for (int b = tid + 2 * MF_BLOCK; b < n_blocks; b += MF_BLOCK) take_record(rec_at(b), b);
    } else {
        take(kreg0);
        take(kreg1);
        take(kreg2);
        for (int c = tid + 3 * MF_BLOCK; c < n_keys; c += MF_BLOCK) take(key_at(c));
    }
    if (sh_q > 0) {                                                  // ... and the descriptors of the frame before that became words
        auto take_sh = [&](uint32_t j, float xs) {
            if (j < (uint32_t)sh_q && xs <= thr && sh_isword(j)) {
                const int slot = atomicAdd(&s_ncand, 1);
                if (slot < RR_KEYS) s_cand[slot] = ((uint64_t)(xs < 0.0f ? 0u : __float_as_uint(xs)) << 32) | (uint64_t)(SHADOW_ROW_BASE + j);
            }
        };
        take_sh(2u * (uint32_t)tid, xsh.x);
        take_sh(2u * (uint32_t)tid + 1u, xsh.y);
        for (int j = 2 * MF_BLOCK + tid; j < sh_q; j += MF_BLOCK) take_sh((uint32_t)j, sh_x[(size_t)qi * sh_ld + j]);   // (frames of more than 512 descriptors)
    }
    lds_barrier();
    RR_STAMP(2);
    const int n_keys_in = s_ncand;
    const bool overflow = n_keys_in > RR_KEYS;
    // A key of the bf16 / fp16 filters stands for a GROUP of four consecutive rows (push_group4: the key's score is the group's minimum, its
    // row the group's first): candidate slot i is row (i & 3) of key i >> 2 -- the four rows of a key are the four 16-lane groups of ONE
    // wave and trip.  A row of the group that is a tombstone, does not exist (yet), or lies at / behind the rows the pending scan covers is
    // no candidate: its exact distance reads +inf.  row_limit: the rows the keys may name (the filter's own row limit when rows are
    // appended on the device -- what lies behind is scanned exactly below --, else the plan's row count).
    const int n_cand = overflow ? n_keys_in : n_keys_in * GS;           // candidate ROWS
    const uint32_t row_limit = (uint32_t)(pend_lo ? p_lo : pend_cap);
    auto cand_row = [&](int i) -> uint32_t { return (uint32_t)s_cand[GS == 4 ? (i >> 2) : i] + (GS == 4 ? (uint32_t)(i & 3) : 0u); };
    // the vocabulary row a LIVE candidate stands for (the distance tie-break is by row): a shadow candidate is the row its descriptor is being
    // written to in this very launch -- behind every row the filter saw, in word order
    auto real_row = [&](int i) -> uint32_t {
        const uint32_t r = cand_row(i);                                   // (a live shadow slot is slot 0 of its key: r = SHADOW_ROW_BASE + j)
        return (sh_q > 0 && r >= SHADOW_ROW_BASE) ? (uint32_t)(n_lo0 + sh_rank(r - SHADOW_ROW_BASE)) : r;
    };

    // ---- exact distances of the candidates (reference arithmetic, dist.h:150-177), one candidate per 16-lane group and trip; the word
    // id of the row is fetched in the same round trip
    float err_ratio = 0.0f;
    if (!overflow) {
        // Two trips in flight (round 6): the rows of trip t + 1 are requested in front of trip t's arithmetic.  A query whose second neighbour is
        // far (a descriptor that will become a word) has dozens of keys under its threshold -- four, five trips of sixteen rows -- and with one
        // trip in flight each was a round trip of its own: those queries' workgroups were the tail of launch B (11.2 us median, 15.5 max).
        auto request = [&](int i, float4& v4, int32_t& wid) {
            const uint64_t key = s_cand[GS == 4 ? (i >> 2) : i];
            const uint32_t row = cand_row(i);
            const bool sh = sh_q > 0 && (uint32_t)key >= SHADOW_ROW_BASE;   // (uniform over the wave: the slots of ONE key) -- a key of ONE row, a word
            const uint32_t sj = (uint32_t)key - SHADOW_ROW_BASE;
            const bool in_range = sh ? (GS == 1 || (i & 3) == 0) : (GS == 1 || row < row_limit);
            const uint32_t rrow = in_range ? row : (uint32_t)key;          // (an address that exists: the group's first row)
            const float* src = sh ? pend_desc + (size_t)sj * DIM : vocab + (size_t)rrow * DIM;
            v4 = reinterpret_cast<const float4*>(src)[lane & 15];
            wid = 0;
            if ((lane & 15) == 0) wid = sh ? pend_id0 + sh_rank(sj) : row_id[rrow];
        };
        auto finish = [&](int i, const float4& v4, int32_t wid) {
            const uint64_t key = s_cand[GS == 4 ? (i >> 2) : i];
            const uint32_t row = cand_row(i);
            const bool sh = sh_q > 0 && (uint32_t)key >= SHADOW_ROW_BASE;
            const bool in_range = sh ? (GS == 1 || (i & 3) == 0) : (GS == 1 || row < row_limit);
            const float t = l2_term4(v4, s_q[lane & 15]);
            float res = 0.0f;
#pragma unroll
            for (int j = 0; j < 16; ++j) res = __fadd_rn(res, __shfl(t, (lane & 48) + j, 64));
            const bool live = in_range && (GS == 1 || __shfl(wid, lane & 48, 64) != 0);
            if (!live) res = __int_as_float(0x7f800000);
            float gmin = res;                                            // the filter's score of a key is its group's minimum (a shadow key: its one row's score)
            if (GS == 4) { gmin = fminf(gmin, __shfl_xor(gmin, 16, 64)); gmin = fminf(gmin, __shfl_xor(gmin, 32, 64)); }
            if ((lane & 15) == 0) {
                s_exact[i] = live ? (((uint64_t)__float_as_uint(res) << 32) | (uint32_t)i) : KEY_NONE;   // the slot stands in for the row: see below
                s_word[i] = wid;
                if (gmin < __int_as_float(0x7f800000)) err_ratio = fmaxf(err_ratio, fabsf(__uint_as_float((uint32_t)(key >> 32)) - gmin) / eps);
            }
        };
        constexpr int STEP = MF_BLOCK / 16;
        // (the trip count is uniform over the WAVE -- the four 16-lane groups of a wave hold the four slots of one key, and n_cand is a multiple
        // of four -- so the shuffles inside finish() always find their lanes)
        int i = tid >> 4;
        float4 va = make_float4(0.f, 0.f, 0.f, 0.f); int32_t wa = 0;
        if (i < n_cand) request(i, va, wa);
        for (; i < n_cand; i += STEP) {
            float4 vb = make_float4(0.f, 0.f, 0.f, 0.f); int32_t wb = 0;
            if (i + STEP < n_cand) request(i + STEP, vb, wb);
            finish(i, va, wa);
            va = vb; wa = wb;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) err_ratio = fmaxf(err_ratio, __shfl_xor(err_ratio, m, 64));
    if (lane == 0) s_err[wave] = err_ratio;
    RR_STAMP(3);

    // ---- pending scan: the two best of the pending rows, from the cross-frame matrix, the staging area or memory
    {
        uint64_t pb = KEY_NONE, ps = KEY_NONE;
        constexpr int PU = 4;                                          // rows per 16-lane group and trip: their loads are in flight together (more
                                                                       // would cost the whole launch -- the scoring workgroups too -- occupancy)
        if (use_cross) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // (each lane reads what its own request brought: no barrier)
            RR_STAMP(4);
            for (int j = tid; j < p_hi - p_lo; j += MF_BLOCK)
                top2_push(pb, ps, ((uint64_t)__float_as_uint(xd[hf * XD_MAX + j]) << 32) | (uint32_t)(p_lo + j));
        } else if (staged) {
            for (int c0 = p_lo; c0 < p_hi_s; c0 += stage_rows) {
                const int n_chunk = min(stage_rows, p_hi_s - c0);
                if (c0 > p_lo) { __syncthreads(); stage_chunk(c0, n_chunk); }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                RR_STAMP(4);
                // ONE LANE PER ROW: the sixteen 4-float terms are formed and added by the same lane in the reference's order (dist.h:150-177),
                // the row's chunks from LDS, the query's as a broadcast read -- no cross-lane traffic (sixteen lanes per row gathered the
                // terms with sixteen ds_bpermute per row: at ~150 pending rows per query that was the whole cost of the scan)
                for (int r = tid; r < n_chunk; r += MF_BLOCK) {
                    float res = 0.0f;
#pragma unroll 4
                    for (int c = 0; c < 16; ++c) res = __fadd_rn(res, l2_term4(*staged_chunk(stage, r, c), s_q[c]));
                    top2_push(pb, ps, ((uint64_t)__float_as_uint(res) << 32) | (uint32_t)(c0 + r));
                }
                if (wr_on && sh_q == 0 && c0 + stage_rows < p_hi) write_rows(c0, n_chunk);   // (more than one chunk: the staging area is about to be reused;
                                                                                // the LAST chunk's rows are written at the very end of the body)
            }
        } else
        for (int base = p_lo; base < (pend_list ? min(p_hi_s, n_lo0) : p_hi_s); base += PU * (MF_BLOCK / 16)) {   // (rows of a deferred append need the staged path)
            float4 v4[PU];
#pragma unroll
            for (int u = 0; u < PU; ++u) {
                const int r0 = base + u * (MF_BLOCK / 16) + (tid >> 4);
                v4[u] = reinterpret_cast<const float4*>(vocab + (size_t)min(r0, p_hi_s - 1) * DIM)[lane & 15];
            }
#pragma unroll
            for (int u = 0; u < PU; ++u) {                             // sixteen lanes per row
                const int r0 = base + u * (MF_BLOCK / 16) + (tid >> 4);
                const float t = l2_term4(v4[u], s_q[lane & 15]);
                float res = 0.0f;
#pragma unroll
                for (int j = 0; j < 16; ++j) res = __fadd_rn(res, __shfl(t, (lane & 48) + j, 64));
                if ((lane & 15) == 0 && r0 < p_hi_s) top2_push(pb, ps, ((uint64_t)__float_as_uint(res) << 32) | (uint32_t)r0);
            }
        }
        if (p_hi_s > p_lo) {                                           // uniform
            wave_top2_reduce(pb, ps);
            if (lane == 0) { s_pend[wave][0] = pb; s_pend[wave][1] = ps; }
        }
    }
    RR_STAMP(5);
    lds_barrier();                                                     // (what the halves hand over lies in LDS; no store is outstanding here)
    RR_STAMP(6);
    asm volatile("" : "+v"(dreg0), "+v"(dreg1));                       // (requested at the top, long since here: no wait for them behind the stores below)

    // ---- top-2: the two best (distance, row) keys; ties go to the lower ROW (result_set.h:151-171), so the comparison key carries the row
    uint64_t best = KEY_NONE, second = KEY_NONE;
    int sbest = -1, ssecond = -1;
    __shared__ int s_below_all[HALVES];                               // (the candidate bits' count of set bits below qi, CandBits::list)
    int& s_below = s_below_all[hf];
    if (wave == 0) {
        if (!overflow)
            for (int i = lane; i < n_cand; i += 64) {
                const uint64_t e = s_exact[i];
                if (e == KEY_NONE) continue;                              // (a row of a key's group that is no candidate)
                top2_push(best, second, (e & 0xFFFFFFFF00000000ull) | real_row((int)(uint32_t)e));
            }
        wave_top2_reduce(best, second);
#ifdef LCD_RR_SUBSTAMP
        RR_STAMP(4);
#endif
        if (p_hi_s > p_lo) {                                           // the pending rows' two best join (their rows differ from every kept key's)
#pragma unroll
            for (int wi = 0; wi < MF_WAVES; ++wi) { top2_push(best, second, s_pend[wi][0]); top2_push(best, second, s_pend[wi][1]); }
        }
        // the second neighbour's distance is all the candidate bits need: it is handed over HERE, and the other waves write their part of the bit
        // row and list while this one looks for the winners' slots, checks the certificate and stores the results (they used to wait for all of that)
        if (lane == 0) {
            s_thr = (cb.have_index && second != KEY_NONE) ? __uint_as_float((uint32_t)(second >> 32)) : __int_as_float(0x7f800000);
            s_below = 0;
        }
    }
    if (cb.bits) lds_barrier();                                        // (uniform; LDS traffic only: no store is outstanding here)
    // ---- winner slots: which candidate slots won (for their word ids; a pending row that won has no slot: -1)
    if (wave == 0) {
        if (!overflow)
            for (int i = lane; i < n_cand; i += 64) {
                if (s_exact[i] == KEY_NONE) continue;
                const uint64_t key = (s_exact[i] & 0xFFFFFFFF00000000ull) | real_row(i);
                if (key == best) sbest = i;
                if (key == second) ssecond = i;
            }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            sbest = max(sbest, __shfl_xor(sbest, m, 64));
            ssecond = max(ssecond, __shfl_xor(ssecond, m, 64));
        }
#ifdef LCD_RR_SUBSTAMP
        RR_STAMP(5);
#endif
    }

    // ---- results and certificate.  The tail of the chain: lane j < 2 of wave 0 holds the query's j-th neighbour (both reductions leave their results
    // in every lane) and writes it -- one store instruction per result array, and ONE round trip for the word ids of winners that have no candidate
    // slot.  Everything that READS memory comes first -- those word ids, the certificate's operands -- and the stores last: the wait counter is one
    // in-order counter for loads and stores, so a load (or the reload of a spilled register) behind a store waits for the store's acknowledgement, a
    // full round trip each time (three of them in the first version of this block: 3.6 us of an 8 us chain, measured with in-kernel stamps).
    if (tid < 2 && valid) {
        err_ratio = fmaxf(fmaxf(s_err[0], s_err[1]), fmaxf(s_err[2], s_err[3]));
        static_assert(MF_WAVES == 4, "the four waves' partial results");
        bound = min(min(s_bound[0], s_bound[1]), min(s_bound[2], s_bound[3]));
        const uint64_t win = tid == 0 ? best : second;
        const int sl = tid == 0 ? sbest : ssecond;
        int32_t wout = 0;
        if (win != KEY_NONE) {
            const int32_t rw = (int32_t)(uint32_t)win;
            wout = sl >= 0 ? s_word[sl] : ((pend_list && rw >= n_lo0) ? pend_id0 + (rw - n_lo0) : row_id[rw]);
        }
        // certificate: every row the filter dropped is strictly farther than the exact second neighbour
        bool ok = !overflow;
        if (ok && bound < INF) {                                      // something finite was dropped
            if (second == KEY_NONE) ok = false;                       // fewer than two exact candidates but rows were dropped
            else ok = __uint_as_float(bound) - eps > __uint_as_float((uint32_t)(second >> 32));
        }
        // the certificate's premise is |filter score - exact distance| <= eps for every row; on the re-ranked candidates that error was
        // just measured: half the budget used up anywhere means the bound is no longer trusted for this query -> exact redo
        if (err_ratio >= 0.5f) ok = false;
        // fp16 operands hold magnitudes up to 65504: descriptors far outside that (the filter multiplies -2 q) are not this filter's
        // business -- the exact scan takes the query
        if (f16 && !(qn < 1.0e8f && vn_max < 1.0e8f)) ok = false;
        const bool report = err_ratio > 0.0f && eps > 0.0f;
        int reject = ok ? 0 : 1;
        asm volatile("" : "+v"(wout), "+v"(reject) :: "memory");   // every load of this thread has arrived: stores only from here
        ok = reject == 0;
        if (tid == 0 && report && __float_as_uint(err_ratio) > err_seen)         // fail_count[2]: max |score - distance| / eps (diagnostics; err_seen above)
            atomicMax(reinterpret_cast<uint32_t*>(fail_count) + 2, __float_as_uint(err_ratio));
        out_row[2 * qi + tid] = win == KEY_NONE ? -1 : (int32_t)(uint32_t)win;
        out_word[2 * qi + tid] = wout;
        out_dist[2 * qi + tid] = win == KEY_NONE ? -1.0f : __uint_as_float((uint32_t)(win >> 32));
        if (tid == 0 && !ok) fail_list[atomicAdd(fail_count, 1)] = qi;
    }
    RR_ACK();
    RR_STAMP(7);

    // ---- candidate bits: the query's row of the candidate bit matrix (uniform branch)
    if (cb.bits) {                                                     // + the compact list of the set bits below qi (CandBits::list)
        // LDS-only barriers from the threshold's hand-over on: wave 0 has just stored the query's results, and __syncthreads() would hold the
        // whole workgroup until those stores are acknowledged -- a memory round trip at the end of a latency chain
        const float thr2 = s_thr;
        for (int base = wave * 64; base < cb.ld; base += MF_BLOCK) {
            const int r = base + lane;
            float d = r == tid ? dreg0 : (r == tid + MF_BLOCK ? dreg1 : __int_as_float(0x7f800000));
            if (r >= 2 * MF_BLOCK && r < cb.nq) d = cb.selfdist[(size_t)qi * cb.ld + r];
            const unsigned long long m = __ballot(d < thr2);
            if (lane == 0 && valid) *reinterpret_cast<unsigned long long*>(cb.bits + (size_t)qi * cb.bw + (base >> 5)) = m;
            if (cb.cnt && d < thr2 && r < qi) {
                const int pos = atomicAdd(&s_below, 1);               // any order: the decision loop takes the two smallest (distance, j)
                if (pos < CAND_LIST && valid) cb.list[(size_t)qi * CAND_LIST + pos] = make_uint2((uint32_t)r, __float_as_uint(d));
            }
        }
        if (cb.cnt) {
            lds_barrier();
            if (tid == 0 && valid) cb.cnt[qi] = s_below;
        }
        RR_TAIL(1, (unsigned long long)n_cand); RR_TAIL(2, (unsigned long long)s_below); RR_TAIL(3, RR_XCD());
    }
    RR_ACK();
    RR_TAIL(0, __builtin_amdgcn_s_memrealtime());

    // ---- row writes and mirror
    if (n_own > 0 && use_cross) {                                      // (every wave has waited for its requests; the rows came with wave 0's, ...)
        __syncthreads();
        write_rows(0, n_own, true);
    }
    if (wr_on && staged && sh_q == 0) {                               // the last (usually the only) chunk is still in the staging area
        const int c0_last = p_lo + ((p_hi - p_lo - 1) / stage_rows) * stage_rows;
        write_rows(c0_last, min(stage_rows, p_hi - c0_last));
    }
    store_mirror();
}
