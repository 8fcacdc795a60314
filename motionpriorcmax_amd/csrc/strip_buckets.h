// Record buckets with chunked spills: the machinery under both voxel-grid builders (voxel.hip, repr.hip).
//
// A binning kernel (256 threads) counts its records per (channel, strip) bucket of its sample in LDS, claims the slots of every
// bucket with ONE global atomic (sb_reserve) and stores 16-byte records {y, x, weight, bucket} (sb_store).  The slots of a
// workgroup that lie beyond the bucket's capacity go to the sample's spill region as ONE contiguous run, named in the sample's
// chunk list.  An accumulate workgroup (1024 threads, one per bucket) visits the bucket's records and -- only if the bucket did
// overflow -- reads the sample's chunk list once (16 bytes per (binning workgroup, overflowed bucket) pair) and then its own
// runs, nothing of the other buckets' spills (sb_drain).  What a record means (its taps, the accumulators) stays with the caller.
//
// A bounds violation (bounds.h) found here is recorded under the including unit's name with a line of THIS file.
#pragma once
#include "common.h"
#include "bounds.h"

struct StripBuckets {
    int NBk, cap;         // buckets = samples x (channels x strips); records a bucket holds
    int spcap, chcap;     // spill records / chunk descriptors per sample
    int *gcount;          // [NBk + 2 B]   fill of every bucket; then per sample: spilled records, chunks
    float4 *rec, *ovf;    // rec [NBk][cap], ovf [B][spcap]
    int4 *chunk;          // [B][chcap]  {bucket within the sample, first spill record, records, -}
};

#ifdef __HIPCC__
// Workgroup of a binning grid (nblk rounded up to 8) that this one stands for, in XCD-contiguous order: the workgroups of an XCD
// (blockIdx.x mod 8) take consecutive parts of the events.  The caller returns if the result is not below nblk.
__device__ __forceinline__ int sb_bin_block(int nblk) {
    const int per = (nblk + 7) >> 3;
    return (blockIdx.x & 7) * per + (blockIdx.x >> 3);
}

// After the barrier behind the LDS counting (s_cnt[i]: this workgroup's records for bucket i of sample b, nloc buckets per sample):
// s_base[i] = first slot of this workgroup in bucket i;  slot - s_spill[i] = place in the sample's spill region, for the slots >= cap.
__device__ __forceinline__ void sb_reserve(const StripBuckets &L, int b, int nloc, const int *s_cnt, int *s_base, int *s_spill) {
    for (int i = threadIdx.x; i < nloc; i += 256) {
        const int c = s_cnt[i];
        const int base = c > 0 ? atomicAdd(&L.gcount[MPC_IDX(b * nloc + i, L.NBk)], c) : 0;
        s_base[i] = base;
        // the slots [max(base, cap), base + c) of this workgroup lie beyond the bucket: ONE run of the sample's spill region,
        // named in the sample's chunk list (the bucket's own workgroup reads the list and then only its runs)
        const int first = max(base, L.cap), nsp = base + c - first;
        if (nsp > 0) {
            const int sp0 = atomicAdd(&L.gcount[L.NBk + 2 * b], nsp);
            const int ci = atomicAdd(&L.gcount[L.NBk + 2 * b + 1], 1);
            MPC_EXPECT(ci < L.chcap);
            if (ci < L.chcap) L.chunk[(size_t)b * L.chcap + MPC_IDX(ci, L.chcap)] = make_int4(i, sp0, nsp, 0);
            s_spill[i] = first - sp0;
        }
    }
    __syncthreads();
}

// the record {y, x, w} of rank `rank` among this workgroup's records for bucket lb of sample b: into the bucket or the spill region
__device__ __forceinline__ void sb_store(const StripBuckets &L, int b, int nloc, int lb, int rank, float y, float x, float w,
                                         const int *s_base, const int *s_spill) {
    const int g = b * nloc + lb;
    const int slot = s_base[MPC_IDX(lb, nloc)] + rank;
    const float4 rec = make_float4(y, x, w, __int_as_float(g));
    if (slot < L.cap) L.rec[MPC_IDX((size_t)g * L.cap + slot, (long long)L.NBk * L.cap)] = rec;
    else {
        const int q = slot - s_spill[MPC_IDX(lb, nloc)];
        MPC_EXPECT(q >= 0 && q < L.spcap);
        if (q >= 0 && q < L.spcap) L.ovf[(size_t)b * L.spcap + q] = rec;
    }
}

// f(record) for every record of bucket g, by the 1024 threads of its accumulate workgroup, in no particular order
template <typename F>
__device__ __forceinline__ void sb_drain(const StripBuckets &L, int g, int nloc, F f) {
    const int tid = threadIdx.x;
    const int filled = L.gcount[MPC_IDX(g, L.NBk)], n = min(filled, L.cap);
    const float4 *rec = L.rec + (size_t)g * L.cap;
    for (int r = tid; r < n; r += 1024) f(rec[r]);
    if (filled > L.cap) {                                 // (workgroup-uniform) this bucket spilled
        const int b = g / nloc, lb = g - b * nloc;
        const int nch = min(L.gcount[L.NBk + 2 * b + 1], L.chcap);
        const int4 *ch = L.chunk + (size_t)b * L.chcap;
        const float4 *ovf = L.ovf + (size_t)b * L.spcap;
        for (int c0 = 0; c0 < nch; c0 += 1024) {          // the chunk list, a descriptor per thread; a wavefront takes the runs its lanes found
            int4 d = make_int4(-1, 0, 0, 0);
            if (c0 + tid < nch) d = ch[MPC_IDX(c0 + tid, L.chcap)];
            unsigned long long mm = __ballot(d.x == lb);
            while (mm != 0ull) {
                const int l = __ffsll((long long)mm) - 1;
                mm &= mm - 1ull;
                const int sp0 = __shfl(d.y, l, 64);
                const int cnt = min(__shfl(d.z, l, 64), max(L.spcap - sp0, 0));
                for (int r = (tid & 63); r < cnt; r += 64) f(ovf[MPC_IDX(sp0 + r, L.spcap)]);
            }
        }
    }
}
#endif

// ---- host side ------------------------------------------------------------------------------
// `bytes` of the workspace at `off`, which moves on by a whole number of granules
template <typename T>
static inline T *sb_take(void *ws, int64_t &off, int64_t bytes) {
    T *p = (T *)((char *)ws + off);
    off += mpc_align(bytes);
    return p;
}

// Sizes for B samples of N events in nloc buckets each, an event making at most per_event records (two channels x its strips), a
// binning workgroup holding wg_events events; then counters, records, spill regions and chunk lists carved from the front of `ws`.
// Returns the bytes taken.
static inline int64_t sb_layout(StripBuckets &L, int B, int64_t N, int64_t nloc, int64_t per_event, int64_t wg_events, void *ws) {
    const int64_t B1 = B > 0 ? B : 1;
    L.NBk = (int)(B * nloc);
    int64_t cap = 4 * ((2 * N + nloc - 1) / nloc);        // four times the mean fill (an event: two channels)
    if (cap < 4096) cap = 4096;
    if (cap > 2 * N) cap = 2 * N;
    L.cap = (int)(cap > 0 ? cap : 1);
    // spill region of a sample: every record it can produce; chunk list: one descriptor per (binning workgroup, bucket it
    // overflowed) -- a binning workgroup holds at most wg_events x per_event records, in at most nloc buckets
    L.spcap = (int)(per_event * N > 0 ? per_event * N : 1);
    const int64_t wg_rec = wg_events * per_event;
    L.chcap = (int)(mpc_cdiv(N > 0 ? N : 1, wg_events) * (nloc < wg_rec ? nloc : wg_rec));
    int64_t off = 0;
    L.gcount = sb_take<int>(ws, off, (L.NBk + 2 * B1 + 8) * 4);
    L.rec = sb_take<float4>(ws, off, (int64_t)L.NBk * L.cap * 16 + 16);
    L.ovf = sb_take<float4>(ws, off, B1 * L.spcap * 16 + 16);
    L.chunk = sb_take<int4>(ws, off, B1 * L.chcap * 16 + 16);
    return off;
}

// every counter to zero, ahead of the binning kernel
static inline int sb_zero_counters(const StripBuckets &L, int B, hipStream_t st) {
    return mpc_zero_async(L.gcount, (size_t)(L.NBk + 2 * B + 8) * 4, st);
}

// the three instantiations of an accumulate kernel may take all of a CU's LDS as dynamic LDS (mpc_raise_lds_cap)
#define SB_LDS_CAP (160 * 1024 - 1024)
