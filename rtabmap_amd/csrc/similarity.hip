// similarity.hip -- kernels and launches of the pair similarity (similarity_body.cuh): Memory::computeLikelihood with
// Kp/TfIdfLikelihoodUsed=false (Memory.cpp:2179-2214) and the comparison of Memory::rehearsal (:4245), i.e. Signature::compareTo's words
// branch of one query against every signature of the index.  Stand-alone launches on the engine stream; the registration, sealing and
// TF-IDF scoring kernels are not involved, and nothing here writes what they read except KeyPool::idf_tab under a stamp of its own.
#include "tfidf.h"
#include "similarity_body.cuh"

#include <algorithm>

namespace lcd {
namespace {

constexpr int SQ_BLOCK = 1024;   // sim_query_kernel (one workgroup)
constexpr int SIM_BLOCK = 512;   // sim_score_kernel

__global__ __launch_bounds__(SQ_BLOCK) void sim_query_kernel(SimQueryArgs a) {
    extern __shared__ uint32_t sq_dyn_smem[];
    sim_query_body<SQ_BLOCK>(sq_dyn_smem, a);
}

// buckets [b0, b0 + gridDim.x): one workgroup each
__global__ __launch_bounds__(TF_R) void sim_slot_nv_kernel(const BucketDev* __restrict__ tab, const uint32_t* __restrict__ bkt_D, int b0,
                                                           uint32_t* __restrict__ slot_nv) {
    sim_slot_nv_body(tab, bkt_D, b0 + (int)blockIdx.x, slot_nv);
}

// every closed bucket (dead ones write zeros) and the open bucket in ONE launch, as score_kernel
__global__ __launch_bounds__(SIM_BLOCK) void sim_score_kernel(SimArgs A) {
    const int g = (int)blockIdx.x;
    if (g < A.n_closed_pad) {                                            // consecutive buckets on one XCD: they share directory lines
        const int b = (g & 7) * (A.n_closed_pad >> 3) + (g >> 3);
        if (b < A.n_closed) sim_sealed_body<SIM_BLOCK>(A, b);
    } else sim_open_body<SIM_BLOCK>(A, g - A.n_closed_pad);
}

__global__ void gather_i32_kernel(const int32_t* __restrict__ dense, const long long* __restrict__ slots, int n, int32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const long long s = slots[i]; out[i] = s >= 0 ? dense[s] : 0; }
}

inline int sim_next_pow2(int v) { int p = 2; while (p < v) p <<= 1; return p; }

}  // namespace

hipError_t launch_gather_i32(const int32_t* dense, const int64_t* slots, int n, int32_t* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    gather_i32_kernel<<<(n + 255) / 256, 256, 0, s>>>(dense, (const long long*)slots, n, out);
    return hipGetLastError();
}

void Similarity::destroy(int64_t* bytes) {
    DevBuf* all[] = {&slot_nv, &q_w, &q_cnt, &q_did, &qd_did, &qd_cnt, &q_meta, &d_int};
    for (DevBuf* d : all) d->release(bytes);
}

hipError_t Similarity::run(Tfidf& t, const int32_t* d_ids, int n, float* out_sim, int32_t* out_pairs, int32_t* out_valid) {
    if (n < 0 || n > TF_MAX_WORDS) return hipErrorInvalidValue;
    if (t.n_slots == 0) return hipSuccess;
    hipStream_t s = t.stream;
    if (!q_w.p) {
        DevBuf* lists[] = {&q_w, &q_cnt, &q_did, &qd_did, &qd_cnt};
        for (DevBuf* d : lists) TF_TRY(d->reserve(TF_MAX_WORDS * 4, 0, s, t.bytes_device));
        TF_TRY(q_meta.reserve(64, 0, s, t.bytes_device));
        // a query of several thousand words needs more than the default 64 KB of dynamic LDS (as the registration's kernels)
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&sim_query_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024) != hipSuccess)
            (void)hipGetLastError();
    }
    TF_TRY(t.flush_retire());                                           // slot_ni of the signatures retired since the last frame
    TF_TRY(t.keys.sync_id2ws());
    // ---- vs of the sealed buckets this call is the first to meet: one launch per run of consecutive buckets
    TF_TRY(grow_zeroed(slot_nv, (size_t)t.buckets.size() * TF_R * 4, s, t.bytes_device));
    const int nb = (int)t.buckets.size();
    for (int b = 0; b < nb;) {
        if (t.buckets[b].state != 1 || t.buckets[b].nv_done) { b += 1; continue; }
        int e = b;
        while (e < nb && t.buckets[e].state == 1 && !t.buckets[e].nv_done) e += 1;
        sim_slot_nv_kernel<<<e - b, TF_R, 0, s>>>(t.bkt_tab.as<BucketDev>(), t.bkt_D.as<uint32_t>(), b, slot_nv.as<uint32_t>());
        TF_TRY(hipGetLastError());
        for (int k = b; k < e; ++k) t.buckets[k].nv_done = true;
        b = e;
    }
    // ---- the query
    t.stamp += 1;                                                       // a stamp no frame has used or will use: the entries a frame left in
    if (t.stamp == 0) t.stamp = 1;                                      // idf_tab go stale exactly as they do when the next frame comes
    SimQueryArgs q;
    q.src = d_ids; q.n = n; q.xlate = t.keys.xlate(); q.xlate_n = t.keys.xlate_n();
    q.H = sim_next_pow2(std::max(2 * n, 128)); q.stamp = t.stamp; q.did = t.keys.did.as<int32_t>();
    q.q_w = q_w.as<uint32_t>(); q.q_cnt = q_cnt.as<uint32_t>(); q.q_did = q_did.as<int32_t>(); q.qd_did = qd_did.as<int32_t>();
    q.qd_cnt = qd_cnt.as<uint32_t>(); q.q_meta = q_meta.as<uint32_t>(); q.tab = t.keys.idf_tab.as<uint2>();
    sim_query_kernel<<<1, SQ_BLOCK, ((size_t)q.H * 2 + 4) * 4, s>>>(q);
    TF_TRY(hipGetLastError());
    // ---- every slot
    const bool has_open = !t.buckets.empty() && t.buckets.back().state == 0;
    SimArgs A;
    A.tab = t.bkt_tab.as<BucketDev>(); A.bkt_D = t.bkt_D.as<uint32_t>(); A.bkt_flags = t.bkt_flags.as<uint32_t>();
    A.dir2 = t.dir2.as<uint32_t>(); A.dir2_stride = t.dir2_stride;
    A.n_closed = nb - (has_open ? 1 : 0);
    A.n_closed_pad = (A.n_closed + 7) / 8 * 8;
    A.n_open_slots = has_open ? t.buckets.back().n_slots : 0;
    A.q_w = q.q_w; A.q_cnt = q.q_cnt; A.q_did = q.q_did; A.qd_did = q.qd_did; A.qd_cnt = q.qd_cnt; A.q_meta = q.q_meta;
    A.slot_ni = t.slot_ni.as<uint32_t>(); A.slot_nv = slot_nv.as<uint32_t>(); A.slot_begin = t.slot_begin.as<uint32_t>();
    A.slot_cnt = t.slot_cnt.as<uint32_t>();
    A.sim_tab = q.tab; A.stamp = q.stamp;
    A.out_sim = out_sim; A.out_pairs = out_pairs; A.out_valid = out_valid;
    const int grid = A.n_closed_pad + (A.n_open_slots + SIM_BLOCK / 64 - 1) / (SIM_BLOCK / 64);
    if (grid > 0) {
        sim_score_kernel<<<grid, SIM_BLOCK, 0, s>>>(A);
        TF_TRY(hipGetLastError());
    }
    launches += 1;
    return hipSuccess;
}

}  // namespace lcd
