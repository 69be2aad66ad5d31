// similarity_body.cuh -- device code of the pair similarity, Signature::compareTo's words branch (Signature.cpp:273-286) over the inverted
// index of tfidf.h:
//   pairs(q, s) = sum over words w > 0 of min(cq(w), cs(w))       cq, cs = occurrences of w in the query / in signature s
//   sim(q, s)   = float(pairs) / float(max(vq, vs))               vq, vs = entries with id > 0; 0 when either is 0
// (EpipolarGeometry::findPairs on two multimaps pairs the k-th occurrence of a word in one with the k-th in the other: min(cq, cs) pairs a
// word.)  Everything up to the one float division is an integer: the result is bit-exact, whatever the order of the sums.
// The traversal is score_body.cuh's -- one workgroup per sealed bucket, one wavefront per signature of the open bucket -- with another
// term: min(count, cq) instead of count x idf, 32-bit sums, and nothing masked by idf (a word every signature holds still pairs).
#pragma once
#include "frame_tail_body.cuh"

namespace lcd {
namespace {

// ---------------------------------------------------------------------------------------------- the query
// One workgroup: the query's word ids -> (postings key, count cq) with an LDS hash (as frame_words_body with do_register == 0), the lists the
// scorer reads, the per-key stamped table {stamp, cq} of the open bucket, and vq.  vq counts EVERY id > 0, also the ids the index has
// never seen: they are valid words of the query that pair with nothing.  LDS: 2 * H + 4 words.
template <int NT>
__device__ __forceinline__ void sim_query_body(uint32_t* smem, const SimQueryArgs& a) {
    const int H = a.H;
    uint32_t* tkey = smem;               // [H] 0xFFFFFFFF = empty
    uint32_t* tcnt = smem + H;           // [H]
    uint32_t* s_misc = tcnt + H;         // [0] unique words, [1] dense words, [2] vq
    const int tid = threadIdx.x;
    for (int i = tid; i < H; i += NT) { tkey[i] = 0xFFFFFFFFu; tcnt[i] = 0u; }
    if (tid < 4) s_misc[tid] = 0u;
    __syncthreads();
    uint32_t valid = 0;
    for (int i = tid; i < a.n; i += NT) {
        const int32_t id = a.src[i];
        if (id <= 0) continue;                                          // "no word" (the reference's "*iter > 0", Memory.cpp:2189)
        valid += 1u;
        const int32_t ws = (long long)id < a.xlate_n ? a.xlate[id] : -1;
        if (ws < 0) continue;                                           // a word no signature of the index ever held
        const uint32_t w = (uint32_t)ws;
        uint32_t h = (w * 2654435761u) & (uint32_t)(H - 1);
        for (;;) {
            const uint32_t old = atomicCAS(&tkey[h], 0xFFFFFFFFu, w);
            if (old == 0xFFFFFFFFu || old == w) { atomicAdd(&tcnt[h], 1u); break; }
            h = (h + 1) & (uint32_t)(H - 1);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) valid += __shfl_xor(valid, off, 64);
    if ((tid & 63) == 0 && valid) atomicAdd(&s_misc[2], valid);
    __syncthreads();
    // the occupied entries in whatever order the table yields: nothing downstream depends on it (integer sums)
    for (int i0 = 0; i0 < H; i0 += NT) {
        const int i = i0 + tid;
        if (i >= H || tkey[i] == 0xFFFFFFFFu) continue;
        const uint32_t w = tkey[i], c = tcnt[i];
        const int32_t d = gload(a.did + w);
        const uint32_t u = atomicAdd(&s_misc[0], 1u);
        a.q_w[u] = w; a.q_cnt[u] = c; a.q_did[u] = d;
        a.tab[w] = make_uint2(a.stamp, c);
        if (d >= 0) {
            const uint32_t j = atomicAdd(&s_misc[1], 1u);
            a.qd_did[j] = d; a.qd_cnt[j] = c;
        }
    }
    __syncthreads();
    if (tid == 0) { a.q_meta[0] = s_misc[0]; a.q_meta[1] = s_misc[1]; a.q_meta[2] = s_misc[2]; }
}

// ---------------------------------------------------------------------------------------------- vs of a sealed bucket
// One workgroup (256 threads): the number of valid words of each of the bucket's 256 signatures = the column sums of its dense rows plus
// the counts of its sparse postings.  Sealed content never changes, so this runs once per bucket (Bucket::nv_done).
__device__ __forceinline__ void sim_slot_nv_body(const BucketDev* __restrict__ tab, const uint32_t* __restrict__ bkt_D, int b, uint32_t* __restrict__ slot_nv) {
    __shared__ uint32_t acc[TF_R];
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    const BucketDev B = tab[b];
    acc[tid] = 0u;
    __syncthreads();
    if (B.state == 1u) {
        const uint32_t D = min(bkt_D[b], B.D_alloc);
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (uint32_t d0 = (uint32_t)wv; d0 < D; d0 += 16u) {           // four rows of a wavefront in flight
            uint32_t c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) c[u] = d0 + 4u * u < D ? gload((const uint32_t*)(B.dense + (size_t)(d0 + 4u * u) * TF_R + 4 * ln)) : 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) { a0 += c[u] & 255u; a1 += (c[u] >> 8) & 255u; a2 += (c[u] >> 16) & 255u; a3 += c[u] >> 24; }
        }
        if (a0) atomicAdd(&acc[4 * ln + 0], a0);
        if (a1) atomicAdd(&acc[4 * ln + 1], a1);
        if (a2) atomicAdd(&acc[4 * ln + 2], a2);
        if (a3) atomicAdd(&acc[4 * ln + 3], a3);
        uint32_t n_sp = 0;
        if (B.W > 0u) {                                                 // the end of the last present word's segment
            const uint2 last = gload2(B.dirb + ((B.W + 31u) / 32u - 1u));
            n_sp = gload(B.sp_off + last.y + (uint32_t)__popc(last.x));
        }
        for (uint32_t e0 = 0; e0 < n_sp; e0 += 4u * TF_R) {
            uint32_t e[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const uint32_t i = e0 + (uint32_t)(u * TF_R + tid); e[u] = i < n_sp ? gload(B.sp_ent + i) : 0u; }
#pragma unroll
            for (int u = 0; u < 4; ++u) if (e[u] & TF_CNT_MASK) atomicAdd(&acc[e[u] >> TF_CNT_BITS], e[u] & TF_CNT_MASK);
        }
    }
    __syncthreads();
    slot_nv[(size_t)b * TF_R + tid] = acc[tid];
}

// ---------------------------------------------------------------------------------------------- scoring
__device__ __forceinline__ void sim_write(const SimArgs& A, long long slot, uint32_t pairs, uint32_t vs, uint32_t vq, uint32_t ni) {
    const bool ok = ni != 0u && vs != 0u && vq != 0u;                   // a retired slot; isBadSignature on either side (Signature.cpp:277)
    A.out_sim[slot] = ok ? __fdiv_rn((float)pairs, (float)max(vq, vs)) : 0.0f;
    if (A.out_pairs) A.out_pairs[slot] = ok ? (int32_t)pairs : 0;
    if (A.out_valid) A.out_valid[slot] = ni != 0u ? (int32_t)vs : 0;
}

// the posting segments of the 64 words of a wavefront, walked by that wavefront alone (score_segments of score_body.cuh): a posting
// contributes min(count, cap), cap = what the query still has of the word
__device__ __forceinline__ void sim_segments(const uint32_t* __restrict__ sp_ent, uint32_t* acc, uint32_t start, uint32_t len, uint32_t cap) {
    const int ln = threadIdx.x & 63;
    uint32_t incl = len;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t y = __shfl_up(incl, off, 64); if (ln >= off) incl += y; }
    const uint32_t Tw = __shfl(incl, 63, 64);                           // wave-uniform
    for (uint32_t t0 = 0; t0 < Tw; t0 += 128) {
        uint32_t e[2], f[2]; bool ok[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const uint32_t t = t0 + (uint32_t)(u * 64 + ln);
            int pos = 0;                                                // number of lanes whose inclusive sum is <= t = the owner of posting t
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1) { const uint32_t v = __shfl(incl, pos + step - 1, 64); if (v <= t) pos += step; }
            if (pos > 63) pos = 63;
            const uint32_t i_o = __shfl(incl, pos, 64), l_o = __shfl(len, pos, 64), s_o = __shfl(start, pos, 64);
            f[u] = __shfl(cap, pos, 64);
            ok[u] = t < Tw;
            e[u] = ok[u] ? gload(sp_ent + s_o + (t - (i_o - l_o))) : 0u;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!ok[u]) continue;
            atomicAdd(&acc[e[u] >> TF_CNT_BITS], min(e[u] & TF_CNT_MASK, f[u]));     // ds_add_u32
        }
    }
}

// start and length of word w's sparse postings in bucket B through the per-bucket directory (saturated records; later passes)
__device__ __forceinline__ void sim_lookup_dirb(const BucketDev& B, uint32_t w, uint32_t& start, uint32_t& len) {
    const uint2 blk = gload2(B.dirb + (w >> 5));
    const uint32_t bit = 1u << (w & 31u);
    if (blk.x & bit) {
        const uint32_t r = blk.y + (uint32_t)__popc(blk.x & (bit - 1u));
        const uint32_t s0 = gload(B.sp_off + r), s1 = gload(B.sp_off + r + 1);
        start = s0; len = s1 - s0;
    }
}

// One workgroup of SCB threads scores one sealed bucket (256 signatures): score_sealed_body's stages.  A sealed bucket keeps a dense
// word's count as min(cs, 255) in the row cell and cs - 255 as a sparse posting, and
//   min(cq, cs) = min(cq, cell) + min(max(cq - 255, 0), excess):
// a dense cell contributes min(cell, cq); a sparse posting of a word WITH a dense row in this bucket is capped at max(cq - 255, 0); every
// other sparse posting (also of a dense word whose id does not fit this bucket's rows) at cq.  LDS: acc[256] u32.
template <int SCB>
__device__ __forceinline__ void sim_sealed_body(const SimArgs& A, int b) {
    __shared__ uint32_t acc[TF_R];
    const int tid = threadIdx.x;
    const BucketDev B = A.tab[b];
    const long long first_slot = (long long)b * TF_R;
    const bool live = B.state == 1u;                                    // a dead bucket has no rows and no directory: every sum stays 0
    constexpr int NWV = SCB / 64;
    constexpr int DR = 128 / NWV > 16 ? 16 : 128 / NWV;
    static_assert(SCB >= 256 && SCB <= 1024 && DR * NWV <= TF_MAX_WORDS, "the unconditional list reads stay inside the buffers");
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63;
    const uint32_t D = live ? min(A.bkt_D[b], B.D_alloc) : 0u;
    const uint32_t BW = live ? B.W : 0u;
    const uint32_t flags = A.bkt_flags[b];
    const int U = (int)A.q_meta[0];
    const int Ud = (int)A.q_meta[1];
    const uint32_t vq = A.q_meta[2];
    // ---- stage A: the query's lists, read without looking at their lengths first (the buffers hold TF_MAX_WORDS entries), ni, vs
    uint32_t w = A.q_w[tid], cq = A.q_cnt[tid]; int32_t did = A.q_did[tid];
    int32_t dj[DR]; uint32_t fj[DR];
#pragma unroll
    for (int u = 0; u < DR; ++u) {
        const int j = wv + u * NWV;                                     // wave-uniform
        dj[u] = A.qd_did[j];
        fj[u] = A.qd_cnt[j];
    }
    if (tid >= U) { w = 0; cq = 0; did = -1; }
#pragma unroll
    for (int u = 0; u < DR; ++u) { if (wv + u * NWV >= Ud) { dj[u] = -1; fj[u] = 0; } }
    const uint32_t ni_v = tid < TF_R ? A.slot_ni[first_slot + tid] : 0u;
    const uint32_t nv_v = tid < TF_R ? A.slot_nv[first_slot + tid] : 0u;
    // ---- stage B: directory records of the words with sparse postings here, dense rows
    const bool dense_here = did >= 0 && (uint32_t)did < D;
    const uint32_t cap = dense_here ? (cq > 255u ? cq - 255u : 0u) : cq;
    const bool look = cap != 0u && w < BW && (!dense_here || (flags & 1u));   // a dense word has sparse postings only for counts > 255
    uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0;
    if (look) {
        const uint4* rec = reinterpret_cast<const uint4*>(A.dir2 + ((size_t)(w >> 5) * A.dir2_stride + (uint32_t)b) * TF_DIR2_DWORDS);
        r0 = gload4(rec); r1 = gload4(rec + 1);
    }
    uint32_t c[DR];
#pragma unroll
    for (int u = 0; u < DR; ++u) c[u] = (dj[u] >= 0 && (uint32_t)dj[u] < D) ? gload((const uint32_t*)(B.dense + (size_t)dj[u] * TF_R + 4 * ln)) : 0u;
    // ---- stage C: start and length of the words' posting segments from the record alone (a block with a count that does not fit its
    //      5-bit field goes through the per-bucket directory)
    uint32_t start = 0, len = 0;
    if (look) {
        const uint32_t f[6] = {r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
        const uint32_t p = w & 31u, pd = p / 6u, ps = 5u * (p % 6u);
        if (!(r0.y & TF_DIR2_SAT)) {
            uint32_t before = 0;
#pragma unroll
            for (uint32_t d = 0; d < 6u; ++d) {
                const uint32_t x = d < pd ? f[d] : (d == pd ? (f[d] & ((1u << ps) - 1u)) : 0u);
                before += dir2_sum6(x);
            }
            uint32_t fd = f[0];
#pragma unroll
            for (uint32_t d = 1; d < 6u; ++d) fd = d == pd ? f[d] : fd;
            len = (fd >> ps) & 31u;
            start = r0.x + before;
        } else sim_lookup_dirb(B, w, start, len);
    }
    // the dense rows: a lane owns four signatures
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
    for (int u = 0; u < DR; ++u) {
        a0 += min(c[u] & 255u, fj[u]); a1 += min((c[u] >> 8) & 255u, fj[u]); a2 += min((c[u] >> 16) & 255u, fj[u]); a3 += min(c[u] >> 24, fj[u]);
    }
    for (int j0 = wv + DR * NWV; j0 < Ud; j0 += DR * NWV) {              // queries with more than 128 dense words
#pragma unroll
        for (int u = 0; u < DR; ++u) {
            const int j = j0 + u * NWV;
            dj[u] = j < Ud ? A.qd_did[j] : -1;
            fj[u] = j < Ud ? A.qd_cnt[j] : 0u;
        }
#pragma unroll
        for (int u = 0; u < DR; ++u) c[u] = (dj[u] >= 0 && (uint32_t)dj[u] < D) ? gload((const uint32_t*)(B.dense + (size_t)dj[u] * TF_R + 4 * ln)) : 0u;
#pragma unroll
        for (int u = 0; u < DR; ++u) {
            a0 += min(c[u] & 255u, fj[u]); a1 += min((c[u] >> 8) & 255u, fj[u]); a2 += min((c[u] >> 16) & 255u, fj[u]); a3 += min(c[u] >> 24, fj[u]);
        }
    }
    for (int i = tid; i < TF_R; i += SCB) acc[i] = 0u;
    __syncthreads();                                                    // accumulators zeroed
    {
        const int ln4 = ln * 4;
        if (a0) atomicAdd(&acc[ln4 + 0], a0);
        if (a1) atomicAdd(&acc[ln4 + 1], a1);
        if (a2) atomicAdd(&acc[ln4 + 2], a2);
        if (a3) atomicAdd(&acc[ln4 + 3], a3);
    }
    // ---- sparse postings, wavefront by wavefront
    sim_segments(B.sp_ent, acc, start, len, cap);
    for (int k0 = SCB; k0 < U; k0 += SCB) {                             // queries with more than SCB unique words
        const int k = k0 + tid;
        uint32_t st2 = 0, ln2 = 0, cap2 = 0;
        if (k < U) {
            const uint32_t w2 = A.q_w[k], cq2 = A.q_cnt[k];
            const int32_t d2 = A.q_did[k];
            const bool dh = d2 >= 0 && (uint32_t)d2 < D;
            cap2 = dh ? (cq2 > 255u ? cq2 - 255u : 0u) : cq2;
            if (cap2 != 0u && w2 < BW && (!dh || (flags & 1u))) sim_lookup_dirb(B, w2, st2, ln2);
        }
        sim_segments(B.sp_ent, acc, st2, ln2, cap2);
    }
    __syncthreads();
    if (tid < TF_R) sim_write(A, first_slot + tid, acc[tid], nv_v, vq, ni_v);
}

// The bucket that is still filling: one wavefront per signature walks the signature's own stretch of the arrival-order log.  vs is the
// sum of all its counts, pairs the sum of min(count, cq) over the entries whose key carries the query's stamp.
template <int SCB>
__device__ __forceinline__ void sim_open_body(const SimArgs& A, int ob) {
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int sl = ob * (SCB / 64) + wv;
    if (sl >= A.n_open_slots) return;
    const BucketDev B = A.tab[A.n_closed];
    const long long slot = (long long)A.n_closed * TF_R + sl;
    const uint32_t begin = A.slot_begin[slot], cnt = A.slot_cnt[slot], ni = A.slot_ni[slot];
    uint32_t pairs = 0, vs = 0;
    if (ni != 0u) {
        for (uint32_t e0 = 0; e0 < cnt; e0 += 4 * 64) {
            uint32_t w[4], pc[4]; uint2 t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t e = e0 + u * 64 + ln;
                w[u] = e < cnt ? gload(B.coo_w + begin + e) : 0xFFFFFFFFu;
                pc[u] = e < cnt ? gload(B.coo_pc + begin + e) : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = A.sim_tab[w[u] != 0xFFFFFFFFu ? w[u] : 0u];      // unconditional: four loads in flight
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (w[u] == 0xFFFFFFFFu) continue;
                const uint32_t cs = pc[u] & TF_CNT_MASK;
                vs += cs;
                if (t[u].x == A.stamp) pairs += min(cs, t[u].y);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { pairs += __shfl_xor(pairs, off, 64); vs += __shfl_xor(vs, off, 64); }
    if (ln == 0) sim_write(A, slot, pairs, vs, A.q_meta[2], ni);
}

}  // namespace
}  // namespace lcd
