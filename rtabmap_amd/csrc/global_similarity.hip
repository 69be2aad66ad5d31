// global_similarity.hip -- Signature::compareTo's global-descriptor branch (Signature.cpp:257-272) of one query against every signature
// slot: the storage owner GlobalRows (tfidf.h), the kernel that streams a channel's row matrix once, and its launches.  Stand-alone launches
// on the engine stream behind the words branch's (similarity.hip), whose result they replace where a channel matches; no other kernel changes.
//
// Arithmetic (include/lcd.h states it as the engine's contract): fp32 products and sums, fused multiply-add.  One wavefront owns one row.
// Lane l adds the elements of the 16-byte vectors l, l + 64, l + 128, ... in ascending index into ONE accumulator; a fixed xor butterfly over
// the 64 lanes follows.  The order is therefore a function of the channel's dim and of nothing else: not of the slot, the number of slots,
// the grid or the entry point (GL_ROWS rows are in flight per wavefront, each with an accumulator of its own).
#include "tfidf.h"

#include <algorithm>

namespace lcd {
namespace {

constexpr int GL_BLOCK = 512;    // 8 wavefronts share one copy of the query row in LDS
constexpr int GL_ROWS = 4;       // rows in flight per wavefront: 4 x 1 KB per step, 16 wavefronts per CU keep 64 KB of HBM loads outstanding

struct GlobArgs {
    const float4* rows; const uint32_t* present; const int32_t* slot_sig;
    const float4* q;                 // the query row of the channel, zero-padded to nvec vectors
    int nvec;                        // stride / 4
    long long n_slots;               // slots to answer
    long long n_have;                // slots the channel's buffers cover (<= n_slots): the rest hold no row
    int first, last;                 // the first / last matching channel of the query, in ascending channel index
    float* sum; int32_t* cnt;        // compareTo's `similarity` and `totalDescs` per slot, carried from channel to channel
    float* out;                      // last: out[slot] = sum / float(cnt) where cnt > 0; untouched (the words-branch value) elsewhere
};

__global__ __launch_bounds__(GL_BLOCK) void glob_dot_kernel(GlobArgs a) {
    extern __shared__ float4 gl_q[];
    for (int v = (int)threadIdx.x; v < a.nvec; v += GL_BLOCK) gl_q[v] = a.q[v];
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    constexpr int WAVES = GL_BLOCK / 64;
    const long long groups = (a.n_slots + GL_ROWS - 1) / GL_ROWS;
    for (long long g = (long long)blockIdx.x * WAVES + wave; g < groups; g += (long long)gridDim.x * WAVES) {
        const long long s0 = g * GL_ROWS;
        bool on[GL_ROWS];
        const float4* rp[GL_ROWS];
        float acc[GL_ROWS];
        bool any_on = false;
#pragma unroll
        for (int r = 0; r < GL_ROWS; ++r) {
            const long long s = s0 + r;
            on[r] = s < a.n_have && a.present[s] != 0u && a.slot_sig[s] != 0;     // retired slots keep their row and score 0
            rp[r] = a.rows + (size_t)(on[r] ? s : 0) * (size_t)a.nvec;            // (a row that exists: what is read there is discarded)
            acc[r] = 0.0f;
            any_on = any_on || on[r];
        }
        if (any_on) {
#pragma unroll 2
            for (int v = lane; v < a.nvec; v += 64) {
                const float4 q = gl_q[v];
                float4 x[GL_ROWS];
#pragma unroll
                for (int r = 0; r < GL_ROWS; ++r) x[r] = rp[r][v];
#pragma unroll
                for (int r = 0; r < GL_ROWS; ++r) {
                    acc[r] = __builtin_fmaf(x[r].x, q.x, acc[r]);
                    acc[r] = __builtin_fmaf(x[r].y, q.y, acc[r]);
                    acc[r] = __builtin_fmaf(x[r].z, q.z, acc[r]);
                    acc[r] = __builtin_fmaf(x[r].w, q.w, acc[r]);
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
                for (int r = 0; r < GL_ROWS; ++r) acc[r] += __shfl_xor(acc[r], off, 64);
        }
        if (lane < GL_ROWS) {                                                     // lane r writes row r
            float my_acc = 0.0f; bool my_on = false;
#pragma unroll
            for (int r = 0; r < GL_ROWS; ++r) if (lane == r) { my_acc = acc[r]; my_on = on[r]; }
            const long long s = s0 + lane;
            if (s < a.n_slots) {
                float similarity = a.first ? 0.0f : a.sum[s];
                int totalDescs = a.first ? 0 : a.cnt[s];
                if (my_on) {
                    const float dotProd = (my_acc + 1.0f) / 2.0f;                 // Signature.cpp:262
                    similarity += dotProd;
                    totalDescs += 1;
                }
                a.sum[s] = similarity;
                a.cnt[s] = totalDescs;
                if (a.last && totalDescs > 0) a.out[s] = similarity / (float)totalDescs;   // :271
            }
        }
    }
}

// row i of src [n x dim] -> row slots[i] (slot0 when slots == NULL) of the channel, the tail up to `stride` zeroed; one workgroup per row
__global__ __launch_bounds__(256) void glob_store_kernel(const float* __restrict__ src, int dim, int stride, const long long* __restrict__ slots,
                                                         long long slot0, long long cap_slots, float* __restrict__ rows, uint32_t* __restrict__ present) {
    const long long s = slots ? slots[blockIdx.x] : slot0;
    if (s < 0 || s >= cap_slots) return;
    const float* from = src + (size_t)blockIdx.x * (size_t)dim;
    float* to = rows + (size_t)s * (size_t)stride;
    for (int j = (int)threadIdx.x; j < stride; j += 256) to[j] = j < dim ? from[j] : 0.0f;
    if (threadIdx.x == 0) present[s] = 1u;
}

}  // namespace

void GlobalRows::destroy(int64_t* bytes) {
    for (Channel& c : ch) { c.rows.release(bytes); c.present.release(bytes); c.dim = c.stride = 0; c.cap_slots = 0; }
    DevBuf* all[] = {&q_rows, &acc_sum, &acc_cnt, &stage};
    for (DevBuf* d : all) d->release(bytes);
}

hipError_t GlobalRows::ensure(Tfidf& t, int c, int dim, int64_t slots, int64_t slots_hint) {
    if (c < 0 || c >= GLOBAL_MAX_CHANNELS || dim < 1 || dim > GLOBAL_MAX_DIM) return hipErrorInvalidValue;
    Channel& C = ch[c];
    if (C.dim && C.dim != dim) return hipErrorInvalidValue;
    if (slots <= C.cap_slots) return hipSuccess;
    const int stride = (dim + 3) & ~3;
    const size_t row_bytes = (size_t)stride * 4;
    const int64_t want = C.cap_slots ? slots : std::max(slots, slots_hint);
    TF_TRY(C.rows.reserve((size_t)want * row_bytes, (size_t)C.cap_slots * row_bytes, t.stream, t.bytes_device));
    TF_TRY(grow_zeroed(C.present, (size_t)want * 4, t.stream, t.bytes_device));
    C.cap_slots = (int64_t)std::min(C.rows.cap / row_bytes, C.present.cap / 4);
    C.dim = dim;
    C.stride = stride;
    return hipSuccess;
}

hipError_t GlobalRows::store(Tfidf& t, int c, const float* d_src, int n, const int64_t* d_slots, int64_t slot0) {
    if (n <= 0) return hipSuccess;
    Channel& C = ch[c];
    glob_store_kernel<<<n, 256, 0, t.stream>>>(d_src, C.dim, C.stride, (const long long*)d_slots, (long long)slot0, (long long)C.cap_slots,
                                               C.rows.as<float>(), C.present.as<uint32_t>());
    return hipGetLastError();
}

hipError_t GlobalRows::clear(Tfidf& t, int c, int64_t slot) {
    Channel& C = ch[c];
    if (!C.dim || slot < 0 || slot >= C.cap_slots) return hipSuccess;            // nothing was ever stored there
    return hipMemsetAsync(C.present.as<uint32_t>() + slot, 0, 4, t.stream);
}

hipError_t GlobalRows::run(Tfidf& t, const GlobalQuery& q, float* out) {
    if (t.n_slots == 0 || !any()) return hipSuccess;                           // no row was ever stored: nothing can match, nothing is allocated
    hipStream_t s = t.stream;
    TF_TRY(acc_sum.reserve((size_t)t.n_slots * 4, 0, s, t.bytes_device));
    TF_TRY(acc_cnt.reserve((size_t)t.n_slots * 4, 0, s, t.bytes_device));
    // the query's channels that can match: type 1 on a channel the handle has stored a row on, ascending
    int act[GLOBAL_MAX_CHANNELS], n_act = 0;
    size_t off[GLOBAL_MAX_CHANNELS], total = 0;
    for (int c = 0; c < q.n && c < GLOBAL_MAX_CHANNELS; ++c) {
        if (q.type[c] != 1 || !ch[c].dim) continue;
        if (q.dim[c] != ch[c].dim || !q.data[c]) return hipErrorInvalidValue;    // (the entry points refuse this before anything runs)
        act[n_act] = c; off[n_act] = total; total += (size_t)ch[c].stride * 4; n_act += 1;
    }
    if (n_act == 0) return hipMemsetAsync(acc_cnt.p, 0, (size_t)t.n_slots * 4, s);
    if (!n_cus) {
        int dev = 0, v = 0;
        TF_TRY(hipGetDevice(&dev));
        TF_TRY(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev));
        n_cus = std::max(v, 1);
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&glob_dot_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, GLOBAL_MAX_DIM * 4) != hipSuccess)
            (void)hipGetLastError();
    }
    TF_TRY(q_rows.reserve(total, 0, s, t.bytes_device));
    TF_TRY(hipMemsetAsync(q_rows.p, 0, total, s));                               // the padding behind dim
    for (int k = 0; k < n_act; ++k)
        TF_TRY(hipMemcpyAsync((char*)q_rows.p + off[k], q.data[act[k]], (size_t)q.dim[act[k]] * 4,
                              q.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    for (int k = 0; k < n_act; ++k) {
        const Channel& C = ch[act[k]];
        GlobArgs a;
        a.rows = C.rows.as<float4>(); a.present = C.present.as<uint32_t>(); a.slot_sig = t.slot_sig.as<int32_t>();
        a.q = (const float4*)((const char*)q_rows.p + off[k]); a.nvec = C.stride / 4;
        a.n_slots = t.n_slots; a.n_have = std::min<int64_t>(t.n_slots, C.cap_slots);
        a.first = k == 0; a.last = k == n_act - 1;
        a.sum = acc_sum.as<float>(); a.cnt = acc_cnt.as<int32_t>(); a.out = out;
        const size_t lds = (size_t)a.nvec * 16;
        const long long groups = (a.n_slots + GL_ROWS - 1) / GL_ROWS, per_block = GL_BLOCK / 64;
        const int per_cu = lds > 40 * 1024 ? 2 : 4;                              // what 160 KB of LDS and 2 048 threads per CU admit
        const long long grid = std::min<long long>((groups + per_block - 1) / per_block, (long long)n_cus * per_cu);
        glob_dot_kernel<<<(unsigned)grid, GL_BLOCK, lds, s>>>(a);
        TF_TRY(hipGetLastError());
    }
    return hipSuccess;
}

}  // namespace lcd
