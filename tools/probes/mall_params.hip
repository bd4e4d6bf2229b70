// Can the 256 MB Infinity Cache keep the two INVARIANT parameter streams (q, b) of the headline pass resident from one pass
// to the next?  (development probe)  The pass reads the last M+1 = 6 iterates of a ring + q + b and writes the next iterate,
// as mall_ring.hip does, but here the ring reads are always non-temporal and only the q/b load policy and the x_d store
// policy vary:
//   q/b policy  nt   global_load ... nt        (what the headline pass does today)
//               def  global_load               (default policy: allocate)
//               sc1  buffer_load ... sc1       (system-coherent-1 bit, via the raw buffer load's aux bits)
//   x_d store   nt / def
// Control: 'rotate 1' points q and b at four rotating copies, so they can never be resident between two uses; the
// difference between a fixed-q/b cell and its rotating twin is the residency effect, not an effect of the load policy.
// Each cell: 8 warm-up launches, then 40 launches timed one by one with events; min / median / max / mean per launch.
// Sizes on the command line (default 1e7 1.3e7 1.6e7: q + b = 160, 208, 256 MB).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
typedef double V2 __attribute__((ext_vector_type(2)));
constexpr int NRING = 6, RING = 8, NCOPY = 4, NT_THREADS = 256;
struct Ptrs { const V2* p[NRING]; const V2* q; const V2* b; V2* out; };
enum { POL_NT = 0, POL_DEF = 1, POL_SC1 = 2 };
__device__ __forceinline__ V2 ld_nt(const V2* p) { return __builtin_nontemporal_load(p); }
template <int POL> __device__ __forceinline__ V2 ldq(const V2* base, __amdgpu_buffer_rsrc_t r, unsigned off) {
    if constexpr (POL == POL_NT) return __builtin_nontemporal_load((const V2*)((const char*)base + off));
    else if constexpr (POL == POL_DEF) return *(const V2*)((const char*)base + off);
    else return __builtin_bit_cast(V2, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 16));   // aux 16 = sc1
}
template <int POL, bool WDEF>
__global__ void __launch_bounds__(NT_THREADS) pass(Ptrs a, unsigned npk, unsigned qbytes) {
    const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)a.q, (short)0, (int)qbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)a.b, (short)0, (int)qbytes, 0x00020000);
    const unsigned stride = gridDim.x * NT_THREADS;
    for (unsigned c = blockIdx.x * NT_THREADS + threadIdx.x; c < npk; c += stride) {
        const unsigned off = c * 16u;
        V2 v[NRING];
#pragma unroll
        for (int s = 0; s < NRING; ++s) v[s] = ld_nt((const V2*)((const char*)a.p[s] + off));
        const V2 q = ldq<POL>(a.q, rq, off), b = ldq<POL>(a.b, rb, off);
        V2 t = q * v[0] - b;
#pragma unroll
        for (int s = 1; s < NRING; ++s) t += v[s];
        V2* o = (V2*)((char*)a.out + off);
        if constexpr (WDEF) *o = t; else __builtin_nontemporal_store(t, o);
    }
}
struct Bufs { V2* ring[RING]; V2* q[NCOPY]; V2* b[NCOPY]; };
template <int POL, bool WDEF>
int run(const Bufs& B, long n, bool rotate, int grid, const char* pname) {
    const unsigned npk = (unsigned)(n / 2), qbytes = (unsigned)(n * 8);
    const int warm = 8, reps = 40;
    std::vector<hipEvent_t> ev(reps + 1);
    for (auto& h : ev) CK(hipEventCreate(&h));
    int k = 0;
    auto launch = [&]() {
        Ptrs a;
        for (int s = 0; s < NRING; ++s) a.p[s] = B.ring[((k - s) % RING + RING) % RING];      // newest first
        const int qc = rotate ? k % NCOPY : 0;
        a.q = B.q[qc]; a.b = B.b[qc];
        a.out = B.ring[(k + 1) % RING];
        hipLaunchKernelGGL((pass<POL, WDEF>), dim3(grid), dim3(NT_THREADS), 0, 0, a, npk, qbytes);
        ++k;
    };
    for (int i = 0; i < warm; ++i) launch();
    CK(hipGetLastError());
    CK(hipEventRecord(ev[0]));
    for (int i = 0; i < reps; ++i) { launch(); CK(hipEventRecord(ev[i + 1])); }
    CK(hipEventSynchronize(ev[reps]));
    std::vector<float> us(reps);
    for (int i = 0; i < reps; ++i) { float ms; CK(hipEventElapsedTime(&ms, ev[i], ev[i + 1])); us[i] = ms * 1e3f; }
    for (auto& h : ev) CK(hipEventDestroy(h));
    double mean = 0;
    for (float u : us) mean += u;
    mean /= reps;
    std::sort(us.begin(), us.end());
    const double med = 0.5 * (us[reps / 2 - 1] + us[reps / 2]);
    printf("n %9ld qb-policy %-3s x_d-store %-3s rotate-qb %d grid %4d : min %7.1f med %7.1f max %7.1f mean %7.1f us  "
           "(spread %4.1f %%, 9 streams: %5.0f GB/s equivalent)\n",
           n, pname, WDEF ? "def" : "nt", rotate ? 1 : 0, grid, us[0], med, us[reps - 1], mean,
           100.0 * (us[reps - 1] - med) / med, 9.0 * n * 8 / med * 1e-3);
    fflush(stdout);
    return 0;
}
int main(int argc, char** argv) {
    std::vector<long> sizes;
    for (int i = 1; i < argc; ++i) sizes.push_back((long)atof(argv[i]));
    if (sizes.empty()) sizes = {10000000L, 13000000L, 16000000L};
    int dev = 0, cus = 0;
    CK(hipGetDevice(&dev));
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    for (long n : sizes) {
        if (n % 2 || n * 8 > 0x7fffffffL) { printf("n %ld: need an even n with n * 8 < 2^31\n", n); return 1; }
        Bufs B;
        for (auto& p : B.ring) { CK(hipMalloc((void**)&p, n * 8)); CK(hipMemset(p, 0, n * 8)); }
        for (int c = 0; c < NCOPY; ++c) {
            CK(hipMalloc((void**)&B.q[c], n * 8)); CK(hipMemset(B.q[c], 0, n * 8));
            CK(hipMalloc((void**)&B.b[c], n * 8)); CK(hipMemset(B.b[c], 0, n * 8));
        }
        CK(hipDeviceSynchronize());
        const int grid = cus;                                     // one 256-thread workgroup per CU, as the headline pass
        int rc = 0;
        for (int rot = 0; rot < 2 && !rc; ++rot) {
            rc |= run<POL_NT, false>(B, n, rot, grid, "nt");
            rc |= run<POL_DEF, false>(B, n, rot, grid, "def");
            rc |= run<POL_SC1, false>(B, n, rot, grid, "sc1");
            rc |= run<POL_NT, true>(B, n, rot, grid, "nt");
            rc |= run<POL_DEF, true>(B, n, rot, grid, "def");
            rc |= run<POL_SC1, true>(B, n, rot, grid, "sc1");
        }
        // second pass over the fixed-q/b cells: the order of the cells must not matter
        rc |= run<POL_NT, false>(B, n, false, grid, "nt");
        rc |= run<POL_DEF, false>(B, n, false, grid, "def");
        for (auto& p : B.ring) CK(hipFree(p));
        for (int c = 0; c < NCOPY; ++c) { CK(hipFree(B.q[c])); CK(hipFree(B.b[c])); }
        if (rc) return rc;
    }
    return 0;
}
