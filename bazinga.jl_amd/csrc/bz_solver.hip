// bz_solver.hip — device-resident PANOCplus / ALPS driver (host side) + kernel launches.
//
// Restates, for the lowered oracle kinds, what the reference runs at
// src/algorithms/alps.jl:64-66: ProximalAlgorithms.PANOCplus(...)(f=alFun, g=gFun, x0=x)
// with alFun = AugLagFun (src/utilities/auglagfun.jl) and gFun = NonsmoothCostFun
// (src/utilities/nonsmoothcostfun.jl).  The scalar control flow below is the same
// as oracle/bazinga_ref.py (PANOCplusIteration.init/step), which documents the
// provenance of the restatement.
#include "bz_solver.h"
#include "bz_spmv.h"
#include "bz_spmm.h"
#include "bz_group.h"
#include "bz_group_ragged.h"
#include "bz_als_dense.h"
#include "bz_csr_host.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <optional>
#include <tuple>
#include <type_traits>

namespace bz {

Ctx::~Ctx() {
    for (int r = 0; r < P2P_MAXRANKS; ++r)
        if (mbox_opened[r] && mbox_peer[r]) (void)hipIpcCloseMemHandle(mbox_peer[r]);
    if (mbox_local) (void)hipFree(mbox_local);
    if (comm) (void)ncclCommDestroy(comm);
    if (stream) (void)hipStreamDestroy(stream);
}

static_assert(sizeof(P2PMailbox) == sizeof(P2PWords), "host and device mailbox layouts differ");

// allocate this rank's mailbox (fine-grained: peers' system-scope stores must be visible to a running
// kernel) and hand out its IPC handle
void p2p_export(Ctx* ctx, void* handle64) {
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "HIP IPC handle is 64 bytes");
    if (ctx->nranks > P2P_MAXRANKS) throw Error(BZ_ERR_ARG, "p2p supports at most 8 ranks");
    BZ_HIP(hipSetDevice(ctx->device));
    if (!ctx->mbox_local) {
        void* p = nullptr;
        BZ_HIP(hipExtMallocWithFlags(&p, sizeof(P2PMailbox), hipDeviceMallocFinegrained));
        BZ_HIP(hipMemset(p, 0, sizeof(P2PMailbox)));
        BZ_HIP(hipDeviceSynchronize());
        ctx->mbox_local = (P2PMailbox*)p;
    }
    hipIpcMemHandle_t h;
    BZ_HIP(hipIpcGetMemHandle(&h, ctx->mbox_local));
    std::memcpy(handle64, &h, sizeof(h));
}

// map every rank's mailbox; from here on scalar exchanges bypass RCCL
void p2p_connect(Ctx* ctx, const void* handles, const int32_t* devices) {
    if (!ctx->mbox_local) throw Error(BZ_ERR_STATE, "bz_ctx_p2p_export must be called first");
    BZ_HIP(hipSetDevice(ctx->device));
    const unsigned char* hs = (const unsigned char*)handles;
    for (int r = 0; r < ctx->nranks; ++r) {
        if (r == ctx->rank) { ctx->mbox_peer[r] = ctx->mbox_local; continue; }
        if (devices && devices[r] == ctx->device) ctx->shared_device = true;
        if (devices && devices[r] != ctx->device) {
            hipError_t e = hipDeviceEnablePeerAccess(devices[r], 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                throw Error(BZ_ERR_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
            (void)hipGetLastError();
        }
        hipIpcMemHandle_t h;
        std::memcpy(&h, hs + (size_t)r * 64, 64);
        void* p = nullptr;
        BZ_HIP(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
        ctx->mbox_peer[r] = (P2PMailbox*)p;
        ctx->mbox_opened[r] = true;
    }
    ctx->p2p_on = true;
}

// ---------------------------------------------------------------------------
// one block per scalar: fold source blockIdx.x and write it to (host-mapped) out
__global__ void __launch_bounds__(BLOCK) k_collect(CollectArgs a, double* out) {
    __shared__ double sh[WAVES];
    const int i = blockIdx.x;
    double t = fold_src(a.src[i], (a.maxmask >> i) & 1u, sh);
    if (threadIdx.x == 0) host_post(out, i, t, a.ticket);
}

// the same for unit-stride sources with ONE wave per scalar (fold_wave gives fold_src's bits): a 64-thread
// workgroup needs no LDS and no barrier
__global__ void __launch_bounds__(64) k_collect_w(CollectArgs a, double* out) {
    const int i = blockIdx.x;
    const double t = fold_wave(a.src[i].p, a.src[i].count, (a.maxmask >> i) & 1u);
    if (threadIdx.x == 0) host_post(out, i, t, a.ticket);
}

// the persistent two-loop kernel's grid barrier gave up (its workgroups were not all resident): single-rank
// solves catch this, switch to the kernel chain for good and redo the iteration
// a pre-launched pass gave up at its gate (the host did not release it in time, or workgroup 0 was not resident in
// time because somebody else holds the CUs): it has written nothing that the same pass, launched again, does not
// write again — single-rank solves catch this, redo the iteration without the gate and leave the gate off
struct GateTimeout : Error {
    explicit GateTimeout(int code) : Error(BZ_ERR_COMM, code == 6 ? "a pre-launched pass timed out at its gate (the host never released it)"
                                                                   : "a pre-launched pass: workgroups timed out waiting for workgroup 0 to open the gate") {}
};
struct DenseFusedTimeout : Error {
    DenseFusedTimeout() : Error(BZ_ERR_HIP, "one-pass dense kernel: a row group's workgroups timed out waiting for each other (not all resident?)") {}
};
struct PersistTimeout : Error {
    PersistTimeout() : Error(BZ_ERR_HIP, "persistent two-loop kernel: grid barrier timed out (blocks not co-resident?)") {}
};

// set by bz_callback_abort() from inside a host callback (callbacks run on the thread that made the library call)
bool& callback_abort_flag() {
    static thread_local bool flag = false;
    return flag;
}

enum Cat : int { C_TWOLOOP = 0, C_FUSED = 1, C_ALGRAD = 2, C_FB = 3, C_UPDATE = 4,
                 C_COLLECT = 5, C_GATHER = 6, C_MISC = 7, C_DOT = 8, C_GEMV = 9, C_PERSIST = 10, C_GEMV_MFMA = 11, C_FUSED_IT = 12,
                 C_STENCIL_FB = 13, C_STENCIL_UPD = 14, C_XD = 15 };

// ---------------------------------------------------------------------------
// Environment knobs (development aids).  Each variable is parsed here, and only here, with the default that
// is measured, at one of three moments: when the problem is created (CreateKnobs), at every bz_panoc_begin (BeginKnobs),
// at every AugLagUpdate! (BZ_UNI).  Constructing a table reads the environment; a table is not changed afterwards: what
// the solver switches at run time (gate_env_ after a gate fallback, the withheld gate release) has members of its own.
static int env_int(const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; }
static long long env_ll(const char* name, long long dflt) { const char* e = std::getenv(name); return e ? std::atoll(e) : dflt; }
static std::optional<int> env_opt(const char* name) { const char* e = std::getenv(name); return e ? std::optional<int>(std::atoi(e)) : std::nullopt; }
struct CreateKnobs {
    std::optional<int> grid = env_opt("BZ_GRID");                        // grid of the streaming kernels
    std::optional<int> persist_blocks = env_opt("BZ_PERSIST_BLOCKS");    // the persistent kernel on b CUs (two ranks on one GPU)
    int dense_fused = env_int("BZ_DENSE_FUSED", 1);      // 0: the dense constraint through two products, not k_dense_fused
    std::optional<int> dense_kp = env_opt("BZ_DENSE_KP");                // k_dense_fused's packs per row and lane
    std::optional<int> spmv_l = env_opt("BZ_SPMV_L");    // lanes per row of the CSR row kernels (a power of two <= 64)
    int spq_fused = env_int("BZ_SPQ_FUSED", 1);          // 0: the sparse quadratic f with c = Identity as product + k_algrad_elem
    int spls_fused = env_int("BZ_SPLS_FUSED", 1);        // 0: the sparse least squares (or logistic) f with c = Identity as two products + k_algrad_elem
    // test-only
    int test_dense_timeout = env_int("BZ_TEST_DENSE_TIMEOUT", 0);        // the k-th k_dense_fused exchange is sabotaged
    unsigned dense_spin = (unsigned)env_ll("BZ_DENSE_SPIN", 0);          // k_dense_fused's poll bound (0: the default)
};
struct BeginKnobs {
    explicit BeginKnobs(int nranks) : gate(env_int("BZ_GATE", nranks > 1 ? 0 : 1)) {}
    int gate;                                    // BZ_GATE: gated pre-launch off (0) / on (non-zero)
    int xr = env_int("BZ_XR", 2);                // one-pass pass on the stored pairs (0) / on the iterates, residuals re-evaluated (non-zero)
    int skipz = env_int("BZ_SKIPZ", 1);          // 0: the one-pass pass always stores z
    int gfc = env_int("BZ_GFC", 0);              // k_fused_compact on k workgroups per CU (0: the per-form default)
    int trialfuse = env_int("BZ_TRIALFUSE", 1);  // 0: a tau-backtracked point finishes in the generic kernels
    int fused_begin = env_int("BZ_FUSED_BEGIN", 1);      // 0: the start of a solve (and ensure_z) in the generic kernels
    int slackfast = env_int("BZ_SLACKFAST", 1);  // 0: the slack iterate-history pass always in its run-time-kinds instantiation
    int slackkind = env_int("BZ_SLACKKIND", 1);  // 0: ... its fast instantiations with run-time kinds of g and D
    int suc_grid = env_int("BZ_SUC_GRID", 1);    // k_stencil_update_c on k workgroups per CU (0: the problem's grid)
    int stencil_regx = env_int("BZ_STENCIL_REGX", 1);    // cfg 3's second pass reads res (0) / re-forms it (1)
    int affine_blend = env_int("BZ_AFFINE_BLEND", 1);    // 0: a tau-backtracked point of cfg 4 always evaluated with a pass over A
    int densesmall = env_int("BZ_DENSESMALL", 1);        // 0: cfg 4's short kernels around the pass over A as launches of their own
    int nt = env_int("BZ_NT", -1);               // non-temporal streams by working-set size (-1) / forced off (0) or on (1)
    int keepp = env_int("BZ_KEEPP", -1);         // q and b of the headline pass cacheable by size (-1, keep_params) / forced
    int ldsq = env_int("BZ_LDSQ", -1);           // the non-temporal fp64 headline pass through its LDS ring (-1, 1) / not (0)
    int famrt = env_int("BZ_FAMRT", 0);          // 1: the headline family through its family-table instantiation
    int spec = env_int("BZ_SPEC", 1);            // 0: k_fused_compact always in its generic instantiation (run-time kinds)
    int xdnt = env_int("BZ_XDNT", 1);            // 0: k_compact_xd, k_stencil_fb, k_stencil_update_c never non-temporal
    bool gemv_valu = std::getenv("BZ_GEMV_VALU") != nullptr;     // set: A'v (fp32) on the vector ALUs, not the MFMA form
    long long persist_min_n = env_ll("BZ_PERSIST_MIN_N", 300000);        // the length from which the persistent kernel runs
    // test-only
    bool test_persist_timeout = env_int("BZ_TEST_PERSIST_TIMEOUT", 0) != 0;      // the persistent kernel's barrier misses its target
    int test_gate_timeout = env_int("BZ_TEST_GATE_TIMEOUT", 0);  // the k-th gate release is withheld
    unsigned gate_spin = (unsigned)env_ll("BZ_GATE_SPIN", 0);    // poll bound of a gated launch's workgroup 0 (0: the default)
};
static int read_uni_knob() { return env_int("BZ_UNI", 2); }      // BZ_UNI=0|1|2, read at every AugLagUpdate! (tests toggle it)

// f(c) with the run-time value as a compile-time constant c (kernel template arguments): a bool, or a UNI (2, 1, else 0)
template <class F> static void with_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <class F> static void with_uni(int u, F&& f) {
    if (u >= 2) f(std::integral_constant<int, 2>{});
    else if (u == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}
// ... or the mode of a row-wise sparse f's pass over A_f (SparseRowF::mode)
template <class F> static void with_sparse_f_mode(int mode, F&& f) {
    switch (mode) {
    case SP_LS_R: f(std::integral_constant<int, SP_LS_R>{}); break;
    case SP_LOGIT_R: f(std::integral_constant<int, SP_LOGIT_R>{}); break;
    case SP_GLM_MODE0 + BZ_LOSS_LEAST_SQUARES: f(std::integral_constant<int, SP_GLM_MODE0 + BZ_LOSS_LEAST_SQUARES>{}); break;
    case SP_GLM_MODE0 + BZ_LOSS_LOGISTIC: f(std::integral_constant<int, SP_GLM_MODE0 + BZ_LOSS_LOGISTIC>{}); break;
    case SP_GLM_MODE0 + BZ_LOSS_HUBER: f(std::integral_constant<int, SP_GLM_MODE0 + BZ_LOSS_HUBER>{}); break;
    case SP_GLM_MODE0 + BZ_LOSS_SQUARED_HINGE: f(std::integral_constant<int, SP_GLM_MODE0 + BZ_LOSS_SQUARED_HINGE>{}); break;
    case SP_GLM_MODE0 + BZ_LOSS_POISSON: f(std::integral_constant<int, SP_GLM_MODE0 + BZ_LOSS_POISSON>{}); break;
    case SPMM_GLM_MODE0 + BZ_LOSS_LEAST_SQUARES: f(std::integral_constant<int, SPMM_GLM_MODE0 + BZ_LOSS_LEAST_SQUARES>{}); break;
    case SPMM_GLM_MODE0 + BZ_LOSS_LOGISTIC: f(std::integral_constant<int, SPMM_GLM_MODE0 + BZ_LOSS_LOGISTIC>{}); break;
    case SPMM_GLM_MODE0 + BZ_LOSS_HUBER: f(std::integral_constant<int, SPMM_GLM_MODE0 + BZ_LOSS_HUBER>{}); break;
    case SPMM_GLM_MODE0 + BZ_LOSS_SQUARED_HINGE: f(std::integral_constant<int, SPMM_GLM_MODE0 + BZ_LOSS_SQUARED_HINGE>{}); break;
    case SPMM_GLM_MODE0 + BZ_LOSS_POISSON: f(std::integral_constant<int, SPMM_GLM_MODE0 + BZ_LOSS_POISSON>{}); break;
    default: f(std::integral_constant<int, SPMM_SOFTMAX>{}); break;
    }
}

template <class T> class Solver final : public SolverBase {
   public:
    Solver(Ctx* c, const bz_problem_desc& d)
        : ctx(c), desc(d), n(d.n), ny(d.ny), nx(d.n), slack(d.slack != 0), env_(c->nranks) {
        if (n <= 0 || ny < 0) throw Error(BZ_ERR_ARG, "n must be positive");
        if (d.c_kind == BZ_C_IDENTITY && ny != n)
            throw Error(BZ_ERR_ARG, "c = Identity requires ny == n");
        ragged_g = d.g_kind == BZ_G_GROUP_LASSO;
        group_g = d.g_kind == BZ_G_NORM_L21 || ragged_g;
        if (ragged_g) {
            // (the group Lasso over a group pointer: a run-time kind beside NormL21, k_fbstep_ragged its one kernel)
            if (d.g_ngroups < 1 || d.g_ngroups > n)
                throw Error(BZ_ERR_ARG, "GroupLasso: g_ngroups must be in 1 .. n");
            if (!d.g_group_ptr) throw Error(BZ_ERR_ARG, "GroupLasso: g_group_ptr (ptr[g_ngroups + 1]) is null");
            if (!d.g_lambda_vec && !(std::isfinite(d.g_lambda) && d.g_lambda >= 0))
                throw Error(BZ_ERR_ARG, "GroupLasso: g_lambda must be finite and >= 0");
            if (!(std::isfinite(d.g_l1) && d.g_l1 >= 0))
                throw Error(BZ_ERR_ARG, "GroupLasso: g_l1 must be finite and >= 0");
            if (slack) throw Error(BZ_ERR_UNSUPPORTED, "GroupLasso: the slack (ALS) form is not lowered with a group penalty");
            if (ctx->nranks > 1) throw Error(BZ_ERR_UNSUPPORTED, "GroupLasso: the group penalty is not sharded (one rank: a shard would have to hold whole groups)");
            if (d.f_kind == BZ_F_CALLBACK || d.c_kind == BZ_C_CALLBACK || d.D_kind == BZ_D_CALLBACK)
                throw Error(BZ_ERR_UNSUPPORTED, "GroupLasso: the group penalty does not mix with host callbacks");
            grp_ng_ = d.g_ngroups;
            grp_ptr_h_.resize((size_t)grp_ng_ + 1);
            BZ_HIP(hipMemcpy(grp_ptr_h_.data(), d.g_group_ptr, grp_ptr_h_.size() * sizeof(int64_t), hipMemcpyDefault));
            if (grp_ptr_h_[0] != 0) throw Error(BZ_ERR_ARG, "GroupLasso: g_group_ptr[0] must be 0");
            grp_max_ = 0;
            for (int64_t j = 0; j < grp_ng_; ++j) {
                const int64_t sz = grp_ptr_h_[j + 1] - grp_ptr_h_[j];
                if (sz < 1)
                    throw Error(BZ_ERR_ARG, "GroupLasso: g_group_ptr must be strictly increasing (group " + std::to_string(j) + " is empty or negative)");
                if (sz > RAGGED_MAX_GROUP)
                    throw Error(BZ_ERR_ARG, "GroupLasso: a group holds 2^30 elements at the most (group " + std::to_string(j) + ")");
                grp_max_ = std::max(grp_max_, sz);
            }
            if (grp_ptr_h_[grp_ng_] != n) throw Error(BZ_ERR_ARG, "GroupLasso: g_group_ptr[g_ngroups] must be n");
            grp_L_ = ragged_lanes(n, grp_ng_);
            // (elements in waves that sweep twice: every group of a wave whose longest group exceeds RAGGED_HOLD trips;
            // with one workgroup trip per group this is the launch's, a function of the pointer alone)
            grp_swept_ = 0;
            const int64_t gpw = 64 / grp_L_;
            for (int64_t w0 = 0; w0 < grp_ng_; w0 += gpw) {
                const int64_t w1 = std::min(grp_ng_, w0 + gpw);
                int64_t mx = 0;
                for (int64_t j = w0; j < w1; ++j) mx = std::max(mx, grp_ptr_h_[j + 1] - grp_ptr_h_[j]);
                if (mx > (int64_t)RAGGED_HOLD * grp_L_) grp_swept_ += grp_ptr_h_[w1] - grp_ptr_h_[w0];
            }
        } else if (d.g_group_ptr) {
            // (g_ngroups and g_l1 are ignored beside every other kind; a pointer is a mistake worth naming)
            throw Error(BZ_ERR_ARG, "g_group_ptr (a group pointer) is taken by GroupLasso alone");
        }
        if (group_g && !ragged_g) {
            // (a run-time kind outside the one-pass family table, as the Lp kinds are: the kernel chain, fbstep() its one prox site)
            if (d.g_group < 1 || d.g_group > 64)
                throw Error(BZ_ERR_ARG, "NormL21: g_group = K must be in 1 .. 64");
            if (n % d.g_group != 0)
                throw Error(BZ_ERR_ARG, "NormL21: n must be a multiple of g_group (x is n / K groups of K)");
            if (!d.g_lambda_vec && !(std::isfinite(d.g_lambda) && d.g_lambda >= 0))
                throw Error(BZ_ERR_ARG, "NormL21: g_lambda must be finite and >= 0");
            if (slack) throw Error(BZ_ERR_UNSUPPORTED, "NormL21: the slack (ALS) form is not lowered with a group penalty");
            if (ctx->nranks > 1) throw Error(BZ_ERR_UNSUPPORTED, "NormL21: the group penalty is not sharded (one rank: a shard would have to hold whole groups)");
            if (d.f_kind == BZ_F_CALLBACK || d.c_kind == BZ_C_CALLBACK || d.D_kind == BZ_D_CALLBACK)
                throw Error(BZ_ERR_UNSUPPORTED, "NormL21: the group penalty does not mix with host callbacks");
            grp_K_ = (int)d.g_group;
            grp_KP_ = 1;
            while (grp_KP_ < grp_K_) grp_KP_ *= 2;
            grp_ng_ = n / grp_K_;
        }
        enet_g = d.g_kind == BZ_G_ELASTIC_NET;
        if (enet_g) {
            // (an element-wise run-time kind outside the one-pass family table: it goes wherever NormL1 with a vector lambda goes)
            if (d.g_lambda_vec)
                throw Error(BZ_ERR_ARG, "ElasticNet: g_lambda_vec must be null (the per-element penalty factors travel in g_weights)");
            enet_check(d.g_lambda, d.g_l2);
        }
        sparse_f = d.f_kind == BZ_F_SPARSE_QUADRATIC;
        if (sparse_f) {
            if (slack) throw Error(BZ_ERR_UNSUPPORTED, "SparseQuadratic: the slack (ALS) form is not lowered with a sparse quadratic f");
            if (d.c_kind == BZ_C_DENSE_AFFINE)
                throw Error(BZ_ERR_UNSUPPORTED, "SparseQuadratic: a sparse quadratic f beside a dense c (DenseAffine) is not lowered");
            if (ctx->nranks > 1) throw Error(BZ_ERR_UNSUPPORTED, "SparseQuadratic: the sparse quadratic f is not sharded (one rank)");
            if (d.g_kind == BZ_G_CALLBACK || d.c_kind == BZ_C_CALLBACK || d.D_kind == BZ_D_CALLBACK)
                throw Error(BZ_ERR_UNSUPPORTED, "SparseQuadratic: the sparse quadratic f does not mix with host callbacks");
            if (!d.f_b || !d.f_sp_rowptr || d.f_sp_nnz < 0 || (d.f_sp_nnz > 0 && (!d.f_sp_col || !d.f_sp_val)))
                throw Error(BZ_ERR_ARG, "SparseQuadratic needs rowptr[n + 1], col[nnz], val[nnz] and q[n]");
            if (n > (int64_t)std::numeric_limits<int32_t>::max())
                throw Error(BZ_ERR_ARG, "SparseQuadratic: n must fit 32-bit column indices");
        }
        // a row-wise sparse f (`sparse_ls`): one row of SPARSE_ROW_F, one set of checks
        for (const SparseRowF& k : SPARSE_ROW_F)
            if (k.f_kind == d.f_kind) { spf_ = k; sparse_ls = true; }
        sparse_mn = d.f_kind == BZ_F_SPARSE_MULTINOMIAL;
        sparse_kw = sparse_mn || d.f_kind == BZ_F_SPARSE_MULTI_GLM;
        const bool glm_loss = d.f_kind == BZ_F_SPARSE_GLM || d.f_kind == BZ_F_SPARSE_MULTI_GLM;      // (a kind that reads f_loss and f_loss_delta)
        if (sparse_ls) {
            sparse_rowwise_check(d);
            if (glm_loss) {
                if (d.f_loss < BZ_LOSS_LEAST_SQUARES || d.f_loss > BZ_LOSS_POISSON)
                    throw Error(BZ_ERR_ARG, std::string(spf_.name) + ": f_loss must be one of BZ_LOSS_* (0 .. 4)");
                if (d.f_loss == BZ_LOSS_HUBER && !(std::isfinite(d.f_loss_delta) && d.f_loss_delta > 0))
                    throw Error(BZ_ERR_ARG, std::string(spf_.name) + ": the Huber loss needs f_loss_delta finite and > 0");
            }
            if (spf_.weighted && !(std::isfinite(d.f_scale) && d.f_scale > 0))
                throw Error(BZ_ERR_ARG, std::string(spf_.name) + ": f_scale must be finite and > 0 (1 for the plain sum)");
            if (d.f_kind == BZ_F_SPARSE_GLM) {
                // the mode follows the loss; without weights and with scale 1 the least-squares and logistic losses ARE the plain
                // kinds and take their epilogues
                spf_.weighted = d.f_w != nullptr || d.f_scale != 1.0 || d.f_loss >= BZ_LOSS_HUBER;
                spf_.mode = spf_.weighted ? SP_GLM_MODE0 + (int)d.f_loss : d.f_loss == BZ_LOSS_LOGISTIC ? SP_LOGIT_R : SP_LS_R;
            }
            // (the multi-response GLM f: always the weighted epilogue, the loss fixing the K-wide mode)
            if (d.f_kind == BZ_F_SPARSE_MULTI_GLM) spf_.mode = SPMM_GLM_MODE0 + (int)d.f_loss;
            if (sparse_kw) {
                // (the three row launches are the K-wide kernels of bz_spmm.h; x is n / K rows of K)
                mn_K_ = (int)d.f_classes;
                mn_KP_ = 2;
                while (mn_KP_ < mn_K_) mn_KP_ *= 2;
            }
        }
        if (d.c_kind == BZ_C_SPARSE_AFFINE) {
            if (slack) throw Error(BZ_ERR_UNSUPPORTED, "SparseAffine: the slack (ALS) form is not lowered with a sparse c");
            if (ctx->nranks > 1) throw Error(BZ_ERR_UNSUPPORTED, "SparseAffine is not sharded (one rank)");
            if (d.D_kind >= BZ_D_VC_PAIRS && d.D_kind <= BZ_D_XOR_PAIRS)
                throw Error(BZ_ERR_UNSUPPORTED, "SparseAffine: pairwise D sets need c = Identity");
            if (d.f_kind == BZ_F_STENCIL5) throw Error(BZ_ERR_UNSUPPORTED, "Stencil5pt f with a sparse c");
            if (d.f_kind == BZ_F_LEAST_SQUARES || d.f_kind == BZ_F_QUADRATIC)
                throw Error(BZ_ERR_UNSUPPORTED, "dense f with a sparse c");
            if (ny <= 0 || !d.c_b || !d.c_sp_rowptr || d.c_sp_nnz < 0 || (d.c_sp_nnz > 0 && (!d.c_sp_col || !d.c_sp_val)))
                throw Error(BZ_ERR_ARG, "SparseAffine needs rowptr[ny + 1], col[nnz], val[nnz] and b[ny]");
            if (n > (int64_t)std::numeric_limits<int32_t>::max() || ny > (int64_t)std::numeric_limits<int32_t>::max())
                throw Error(BZ_ERR_ARG, "SparseAffine: n and ny must fit 32-bit column indices");
        }
        if (slack) {
            // ALS: the inner solver works on xs = [x; s]; from here on `n` is the length of that vector
            // (c = Identity: x_i pairs with s_i, element-wise f ; c = DenseAffine: halves of unequal length, f element-wise
            // or dense, the generic kernel chain around two passes over A)
            const bool f_elem = d.f_kind == BZ_F_ZERO || d.f_kind == BZ_F_DIAG_QUADRATIC;
            const bool f_dense = d.f_kind == BZ_F_LEAST_SQUARES || d.f_kind == BZ_F_QUADRATIC;
            if (!((d.c_kind == BZ_C_IDENTITY && f_elem) || (d.c_kind == BZ_C_DENSE_AFFINE && (f_elem || f_dense))))
                throw Error(BZ_ERR_UNSUPPORTED, "slack (ALS) form: c = Identity with an element-wise f, or c = DenseAffine with an "
                                                "element-wise or dense f (no Stencil5pt f, no callbacks)");
            if (nx % PackN<T>::N != 0)
                throw Error(BZ_ERR_ARG, "slack (ALS) form: n must be a multiple of 16 bytes");
            if (ctx->nranks > 1) throw Error(BZ_ERR_UNSUPPORTED, "slack (ALS) form is not sharded");
            n = nx + ny;
        }
        {
            // generic (user-defined) oracles: host callbacks, all four together
            const int ncb = (d.f_kind == BZ_F_CALLBACK) + (d.g_kind == BZ_G_CALLBACK) + (d.c_kind == BZ_C_CALLBACK) +
                            (d.D_kind == BZ_D_CALLBACK);
            if (ncb != 0 && ncb != 4)
                throw Error(BZ_ERR_ARG, "generic oracles: f, g, c and D must all be the CALLBACK kind together");
            generic_ = ncb == 4;
            if (generic_) {
                if (!d.cb_f_gradient || !d.cb_g_prox || !d.cb_c_eval || !d.cb_c_jtprod || !d.cb_D_proj)
                    throw Error(BZ_ERR_ARG, "generic oracles: a callback pointer is null");
                if (slack || ctx->nranks > 1)
                    throw Error(BZ_ERR_UNSUPPORTED, "generic oracles: single rank, no slack form");
                if (ny <= 0) throw Error(BZ_ERR_ARG, "generic oracles: ny must be positive");
            }
        }
        if (d.c_kind != BZ_C_IDENTITY && d.c_kind != BZ_C_DENSE_AFFINE && d.c_kind != BZ_C_SPARSE_AFFINE && !generic_)
            throw Error(BZ_ERR_UNSUPPORTED, "constraint kind not lowered to the device");
        if (d.c_kind == BZ_C_DENSE_AFFINE) {
            if (ny <= 0 || !d.c_A || !d.c_b) throw Error(BZ_ERR_ARG, "DenseAffine needs A[ny][n] and b[ny]");
            if (d.f_kind == BZ_F_STENCIL5) throw Error(BZ_ERR_UNSUPPORTED, "Stencil5pt f with a dense c");
            // nranks > 1: the ROWS of A (and b, mu, y: ny = this rank's rows) are sharded, x is replicated; the
            // n-vector A' yhat is summed over the ranks through IPC-mapped regions (bz_problem_allreduce_*)
            if (ctx->nranks > 1 && (!ctx->p2p_on || slack))
                throw Error(BZ_ERR_UNSUPPORTED, "a row-sharded DenseAffine needs the p2p mailboxes and no slack");
        }
        if ((d.f_kind < BZ_F_ZERO || d.f_kind > BZ_F_QUADRATIC) && !sparse_f && !sparse_ls && !generic_)
            throw Error(BZ_ERR_UNSUPPORTED, "smooth-cost kind not lowered to the device");
        dense_f = d.f_kind == BZ_F_LEAST_SQUARES || d.f_kind == BZ_F_QUADRATIC;
        if (dense_f) {
            if (!d.f_A || !d.f_b || d.f_rows <= 0) throw Error(BZ_ERR_ARG, "dense f needs its matrix, vector and row count");
            if (d.f_kind == BZ_F_QUADRATIC && d.f_rows != nx) throw Error(BZ_ERR_ARG, "Quadratic: Q must be n-by-n");
            if (d.c_kind != BZ_C_IDENTITY && d.c_kind != BZ_C_DENSE_AFFINE)
                throw Error(BZ_ERR_UNSUPPORTED, "dense f needs c = Identity or c = DenseAffine");
            if (ctx->nranks > 1) throw Error(BZ_ERR_UNSUPPORTED, "dense f is not sharded");
        }
        if (d.f_kind == BZ_F_STENCIL5) {
            if (d.f_grid_nx <= 0 || d.f_grid_ny <= 0 || d.f_grid_nx * d.f_grid_ny != n)
                throw Error(BZ_ERR_ARG, "Stencil5pt: grid nx*ny must equal n");
            if (d.f_grid_ny % PackN<T>::N != 0)
                throw Error(BZ_ERR_ARG, "Stencil5pt: grid columns must be a multiple of 16 bytes");
            // nranks > 1: the grid is sharded by row blocks in rank order (f_grid_nx = this rank's rows); the
            // halo rows travel through IPC-mapped buffers (bz_problem_halo_export / _connect)
            if (ctx->nranks > 1 && !ctx->p2p_on)
                throw Error(BZ_ERR_UNSUPPORTED, "a sharded Stencil5pt needs the p2p mailboxes (bz_ctx_p2p_connect)");
        }
        if ((d.g_kind < BZ_G_ZERO || d.g_kind > BZ_G_NORM_LP_BOX) && !group_g && !enet_g && !generic_)
            throw Error(BZ_ERR_ARG, "unknown g kind");
        if ((d.D_kind < BZ_D_ZERO || d.D_kind > BZ_D_XOR_PAIRS) && !generic_) throw Error(BZ_ERR_ARG, "unknown D kind");
        if (d.D_kind >= BZ_D_VC_PAIRS && d.D_kind <= BZ_D_XOR_PAIRS) {
            // adjacent pairs live inside one 16-byte pack: only the element-wise kernels (c = Identity) see them
            if (d.c_kind != BZ_C_IDENTITY || slack || d.f_kind == BZ_F_STENCIL5)
                throw Error(BZ_ERR_UNSUPPORTED, "pairwise D sets need c = Identity, an element-wise or dense f and no slack");
            if (ny % 2 != 0) throw Error(BZ_ERR_ARG, "pairwise D sets need an even number of constraints");
        }
        // (a per-element lambda: NormL1 alone — the box kinds use the one spare per-element g stream for u, and the
        // reference's NormL1Nonneg takes a number; g_lambda is ignored beside it)
        if (d.g_lambda_vec && d.g_kind != BZ_G_NORM_L1 && !group_g)
            throw Error(BZ_ERR_ARG, "g_lambda_vec (a per-element lambda) is taken by NormL1 alone");
        if ((d.g_kind == BZ_G_NORM_L1 || d.g_kind == BZ_G_NORM_L1_NONNEG ||
             d.g_kind == BZ_G_NORM_L1_BOX || d.g_kind == BZ_G_NORM_L0_BOX) && d.g_lambda < 0 && !d.g_lambda_vec)
            throw Error(BZ_ERR_ARG, "parameter lambda must be nonnegative");
        BZ_HIP(hipSetDevice(ctx->device));
        const int64_t nchunks = (n + PackN<T>::N - 1) / PackN<T>::N;
        {
            hipDeviceProp_t prop;
            BZ_HIP(hipGetDeviceProperties(&prop, ctx->device));
            num_cus = prop.multiProcessorCount;
            pblocks = num_cus;
            // BZ_PERSIST_BLOCKS: run the persistent kernel on fewer CUs (two ranks sharing one GPU in tests)
            if (cenv_.persist_blocks) pblocks = std::max(1, std::min(num_cus, *cenv_.persist_blocks));
            // persistent two-loop: one 512-thread block per CU, KR register packs per thread; its vectors
            // are zero-padded to KR*num_cus*512 packs so that every round is in-bounds (no masks)
            const int64_t kneed = (nchunks + (int64_t)pblocks * PBLOCK - 1) / ((int64_t)pblocks * PBLOCK);
            persist_kr = (kneed <= 48 && pblocks > 0 && pblocks <= PSTRIDE) ? persist_round_kr((int)kneed) : 0;
            // the hand-rolled grid barrier needs every workgroup resident at once: ask the runtime how many 512-thread
            // workgroups of this instantiation fit a CU (a non-resident grid would spin until the bounded polls give
            // up; that case — another process or stream holding CUs — is caught at run time, see step())
            if (persist_kr && persist_occupancy(persist_kr) * num_cus < pblocks) persist_kr = 0;
            vcap = n;
            if (persist_kr) vcap = std::max<int64_t>(n, (int64_t)persist_kr * pblocks * PBLOCK * PackN<T>::N);
        }
        int g = (int)std::min<int64_t>(PSTRIDE, std::max<int64_t>(1, (nchunks + BLOCK - 1) / BLOCK));
        if (cenv_.grid) g = std::max(1, std::min(PSTRIDE, *cenv_.grid));
        grid = g;
        const int64_t nychunks = (ny + PackN<T>::N - 1) / PackN<T>::N;
        grid_y = (int)std::min<int64_t>(grid, std::max<int64_t>(1, (nychunks + BLOCK - 1) / BLOCK));
        if (d.c_kind == BZ_C_IDENTITY) grid_y = grid;
        grid_x = grid;
        slack_dense = slack && d.c_kind == BZ_C_DENSE_AFFINE;
        if (slack) {
            // kernels over the x half alone (and, with c = Identity, over the index both halves share)
            const int64_t c2 = (nx / PackN<T>::N + BLOCK - 1) / BLOCK;
            grid_x = (int)std::min<int64_t>(PSTRIDE, std::max<int64_t>(1, c2));
            if (!slack_dense) grid_y = grid_x;
            lifted_sections(nx, ny, lgx_, lgs_);
        }
        npad = ((n + PackN<T>::N - 1) / PackN<T>::N) * PackN<T>::N;
        npadx = ((nx + PackN<T>::N - 1) / PackN<T>::N) * PackN<T>::N;      // (the matrices of f and c have nx columns)
        if (dense_f) {
            frows = d.f_rows;
            FA_.alloc((size_t)frows * nx);
            BZ_HIP(hipMemcpyAsync(FA_.p, d.f_A, (size_t)frows * nx * sizeof(T), hipMemcpyDefault, ctx->stream));
            BZ_HIP(hipStreamSynchronize(ctx->stream));
            upload(fb_, d.f_b, d.f_kind == BZ_F_LEAST_SQUARES ? frows : nx);
            FR_.alloc(std::max<int64_t>(frows, nx));
            fscale = d.f_kind == BZ_F_LEAST_SQUARES ? T(0.5) : T(1);
            if (d.f_kind == BZ_F_LEAST_SQUARES) {
                // (f's matrix has its own chunk plan and its own partials: f_rows, ny and n are unrelated)
                DFX_.alloc(npadx);
                plan_chunks(frows, nx, f_rows_per_chunk, f_nrowchunks);
                FGT_.alloc((size_t)f_nrowchunks * npadx);
            }
        }
        if (sparse_f) {
            // (the generic kernel chain: no one-pass family kernel, no affine images, no k_begin_lip)
            sparse_f_create(d);
            upload(fb_, d.f_b, nx);
            FR_.alloc(nx);
        }
        if (sparse_ls) {
            // (the generic kernel chain too; the two least-squares modes keep the value convention of the dense LeastSquares: sum
            // r^2, halved by fscale ; every other mode: the plain sum of the rows' losses)
            frows = d.f_rows;
            sparse_ls_create(d);
            // (the multi-response GLM f: B is m rows of K ; both K-wide kinds: R is m rows of K)
            upload(fb_, d.f_b, d.f_kind == BZ_F_SPARSE_MULTI_GLM ? frows * mn_K_ : frows);
            FR_.alloc(sparse_kw ? frows * mn_K_ : frows);
            if (d.c_kind == BZ_C_SPARSE_AFFINE || !spls_fused_on()) DFX_.alloc(nx);
            fscale = spf_.mode == SP_LS_R || spf_.mode == SP_GLM_MODE0 + BZ_LOSS_LEAST_SQUARES ||
                             spf_.mode == SPMM_GLM_MODE0 + BZ_LOSS_LEAST_SQUARES ? T(0.5) : T(1);
            if (sparse_mn) mn_labels_check(d);
            if (d.f_kind == BZ_F_SPARSE_GLM || sparse_kw) glm_weights_create(d);
        }
        if (d.c_kind == BZ_C_DENSE_AFFINE) {
            A_.alloc((size_t)ny * nx);
            BZ_HIP(hipMemcpyAsync(A_.p, d.c_A, (size_t)ny * nx * sizeof(T), hipMemcpyDefault, ctx->stream));
            BZ_HIP(hipStreamSynchronize(ctx->stream));
            upload(cb_, d.c_b, ny);
            CX_.alloc(ny); YU_.alloc(ny);
            plan_chunks(ny, nx, rows_per_chunk, nrowchunks);
            x_replicated = ctx->nranks > 1;
            dense_fused_plan();
            GT_.alloc((size_t)std::max(nrowchunks, df_groups_) * npadx);
            if (x_replicated) JL_.alloc(npad);
            affine_ok_ = !x_replicated && !slack && (d.D_kind == BZ_D_ZERO || d.D_kind == BZ_D_FREE) &&
                         (d.f_kind == BZ_F_ZERO || d.f_kind == BZ_F_DIAG_QUADRATIC);
            if (affine_ok_) {
                CXS_.alloc(ny); CZS_.alloc(ny); CXD_.alloc(ny); CZN_.alloc(ny);
            }
        }
        if (d.c_kind == BZ_C_SPARSE_AFFINE) {
            sparse_create(d);
            upload(cb_, d.c_b, ny);
            CX_.alloc(ny); YU_.alloc(ny);
        }

        std::memset(&P, 0, sizeof(P));
        P.f_kind = d.f_kind; P.g_kind = d.g_kind; P.D_kind = d.D_kind;
        if (d.f_kind == BZ_F_DIAG_QUADRATIC) {
            if (!d.f_q || !d.f_b) throw Error(BZ_ERR_ARG, "DiagQuadratic needs q and b");
            upload(q_, d.f_q, nx); upload(b_, d.f_b, nx);
            P.q = q_.p; P.b = b_.p;
        }
        if (dense_f || sparse_f) P.b = fb_.p;              // Quadratic: q, read by the element-wise kernels and the row epilogues
        if (d.f_kind == BZ_F_STENCIL5) {
            if (!d.f_b) throw Error(BZ_ERR_ARG, "Stencil5pt needs b");
            upload(b_, d.f_b, n);
            P.b = b_.p;
        }
        P.g_lambda = (T)d.g_lambda;
        if (d.g_lambda_vec && group_g) {
            // (one entry per group, in the union slot g_u and NormL1's vector share: read through P.group_lambda_vec())
            std::vector<T> lam;
            read_group_lambda_vec(d.g_lambda_vec, lam);
            upload(glam_, lam.data(), grp_ng_); P.g_group_lambda = glam_.p;
        } else if (d.g_lambda_vec) {
            // (the x half in the slack form: the s half has no g)
            std::vector<T> lam;
            read_lambda_vec(d.g_lambda_vec, lam);
            upload(glam_, lam.data(), nx); P.g_lambda_vec = glam_.p;      // (shares its slot with g_u: read through P.lambda_vec())
        }
        if (ragged_g) {
            gptr_.alloc((size_t)grp_ng_ + 1);
            BZ_HIP(hipMemcpyAsync(gptr_.p, grp_ptr_h_.data(), grp_ptr_h_.size() * sizeof(int64_t), hipMemcpyDefault, ctx->stream));
            BZ_HIP(hipStreamSynchronize(ctx->stream));
        }
        P.g_p = (T)d.g_p;
        lp_g = d.g_kind == BZ_G_NORM_LP_NONNEG || d.g_kind == BZ_G_NORM_LP_BOX;
        if (lp_g) {
            if (!(d.g_p > 0)) throw Error(BZ_ERR_ARG, "p must be positive");
            if (!(d.g_p < 1)) throw Error(BZ_ERR_ARG, "p must be smaller than one");
            if (d.g_lambda < 0) throw Error(BZ_ERR_ARG, "alpha must be nonnegative");
        }
        if (d.g_kind == BZ_G_NORM_L1_BOX || d.g_kind == BZ_G_NORM_L0_BOX || d.g_kind == BZ_G_NORM_LP_BOX) {
            if (!d.g_u) throw Error(BZ_ERR_ARG, "NormL1Box / NormL0Box / NormLpPowerBox need u");
            upload(gu_, d.g_u, nx); P.g_u = gu_.p;
        }
        P.g_lo = (T)d.g_lo; P.g_hi = (T)d.g_hi;
        if (enet_g) {
            // (gamma * 1 is gamma: the kernels' gl is the arm's t; l1 and l2 travel where a box's bounds do, see ElemParams::g_weights)
            P.g_lambda = T(1); P.g_lo = (T)d.g_lambda; P.g_hi = (T)d.g_l2;
            if (d.g_weights) {
                // (the x half in the slack form: the s half has no g)
                std::vector<T> w;
                read_elem_vec(d.g_weights, w, "ElasticNet", "g_weights");
                upload(glam_, w.data(), nx); P.g_weights = glam_.p;      // (shares its slot with g_u: read through P.weights())
            }
        }
        if (d.g_kind == BZ_G_IND_BOX) {
            if (d.g_lo_vec) { upload(glo_, d.g_lo_vec, nx); P.g_lo_vec = glo_.p; }
            if (d.g_hi_vec) { upload(ghi_, d.g_hi_vec, nx); P.g_hi_vec = ghi_.p; }
        }
        P.D_lo = (T)d.D_lo; P.D_hi = (T)d.D_hi;
        if (d.D_kind == BZ_D_BOX) {
            if (d.D_lo_vec) { upload(dlo_, d.D_lo_vec, ny); P.D_lo_vec = dlo_.p; }
            if (d.D_hi_vec) { upload(dhi_, d.D_hi_vec, ny); P.D_hi_vec = dhi_.p; }
        }
        mu_.alloc(ny); muy_.alloc(ny); ymul_.alloc(ny); sproj_.alloc(ny);
        if (generic_) {
            const size_t nn = (size_t)std::max<int64_t>(n, ny);
            for (auto* v : {&hx_, &hg_, &hy_, &hz_, &hres_, &hdfx_, &hjtv_}) v->assign(nn, T(0));
            for (auto* v : {&hcx_, &ht_, &hs_, &hmu_, &hmuy_, &hyv_}) v->assign((size_t)ny, T(0));
        }
        P.mu = mu_.p; P.muy = muy_.p;
        for (auto& b : X_) b.alloc(vcap);
        for (auto& b : RES_) b.alloc(vcap);
        for (auto& b : Z_) b.alloc(vcap);
        GX_.alloc(vcap); GZ_.alloc(vcap); D_.alloc(vcap); TMP_.alloc(vcap);
        if (affine_ok_) { GXN_.alloc(vcap); GZN_.alloc(vcap); }
        parts_.alloc((size_t)SL_COUNT * PSTRIDE);
        BZ_HIP(hipMemsetAsync(parts_.p, 0, (size_t)SL_COUNT * PSTRIDE * sizeof(double), ctx->stream));
        alphas_.alloc(MAX_MEM + 1);
        send_.alloc(SL_COUNT);
        recv_.alloc((size_t)SL_COUNT * std::max(1, ctx->nranks));
        BZ_HIP(hipHostMalloc((void**)&host_out_, sizeof(double) * 2 * MAX_COLLECT, hipHostMallocMapped));
        std::memset(host_out_, 0, sizeof(double) * 2 * MAX_COLLECT);
        BZ_HIP(hipHostGetDevicePointer((void**)&host_out_dev_, host_out_, 0));
        BZ_HIP(hipHostMalloc((void**)&ptimeout_, sizeof(int), hipHostMallocMapped));
        *ptimeout_ = 0;
        BZ_HIP(hipHostGetDevicePointer((void**)&ptimeout_dev_, ptimeout_, 0));
        pcounter_.alloc(PSHARDS * PSHARD_STRIDE);      // zero-filled by alloc
        pgflag_.alloc(2); pglobal_.alloc(4);
        for (int s = 0; s < SL_COUNT; ++s) { grp_first[s] = s; grp_cnt[s] = 1; slot_n[s] = grid; }
        slot_n[SL_OUTER] = slot_n[SL_OUTER + 1] = grid_y;
        BZ_HIP(hipStreamSynchronize(ctx->stream));
    }

    ~Solver() override {
        gate_abort();
        (void)hipStreamSynchronize(ctx->stream);
        if (gate_host_) (void)hipHostFree(gate_host_);
        for (auto& r : prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        for (auto& e : ev_pool) (void)hipEventDestroy(e);
        for (int r = 0; r < P2P_MAXRANKS; ++r)
            if (ar_peer_[r] && ar_peer_[r] != ar_local_) (void)hipIpcCloseMemHandle(ar_peer_[r]);
        if (ar_local_) (void)hipFree(ar_local_);
        if (halo_prev_) (void)hipIpcCloseMemHandle(halo_prev_);
        if (halo_next_) (void)hipIpcCloseMemHandle(halo_next_);
        if (halo_local_) (void)hipFree(halo_local_);
        if (host_out_) (void)hipHostFree(host_out_);
        if (ptimeout_) (void)hipHostFree(ptimeout_);
    }

    // ------------------------------------------------------------------ API
    // lambda of a live problem, between solves.  Number <-> vector would change which kernel forms the problem runs: that
    // stays a creation-time decision.  Every launch takes P as it is when it is made and g_value reads P, so nothing else
    // holds a copy — but a one-pass launch made early for an iteration that never came, which is recalled here.
    void set_g_lambda(double lam, const void* lam_vec) override {
        const int k = desc.g_kind;
        if (group_g) { set_group_lambda(lam, lam_vec); return; }
        if (!(k == BZ_G_NORM_L1 || k == BZ_G_NORM_L1_NONNEG || k == BZ_G_NORM_L1_BOX || k == BZ_G_NORM_L0_BOX))
            throw Error(BZ_ERR_ARG, "bz_problem_set_g_lambda: g must be NormL1, NormL1Nonneg, NormL1Box or NormL0Box");
        if (lam_vec && !P.lambda_vec())
            throw Error(BZ_ERR_ARG, "bz_problem_set_g_lambda: the problem was created with a number lambda (NormL1 takes a vector at bz_problem_create only)");
        if (!lam_vec && P.lambda_vec())
            throw Error(BZ_ERR_ARG, "bz_problem_set_g_lambda: the problem was created with a vector lambda of NormL1: pass a vector");
        std::vector<T> h;
        if (lam_vec) read_lambda_vec(lam_vec, h);
        else if (lam < 0) throw Error(BZ_ERR_ARG, "parameter lambda must be nonnegative");
        gate_abort();
        BZ_HIP(hipStreamSynchronize(ctx->stream));
        if (lam_vec) copy_in(glam_.p, h.data(), nx);
        else { P.g_lambda = (T)lam; desc.g_lambda = lam; }
    }
    // l1 and l2 of a live ElasticNet problem, between solves; the weights stay.  As set_g_lambda: P is all that holds them.
    void set_g_elastic_net(double l1, double l2) override {
        if (!enet_g) throw Error(BZ_ERR_ARG, "bz_problem_set_g_elastic_net: g must be ElasticNet");
        enet_check(l1, l2);
        gate_abort();
        BZ_HIP(hipStreamSynchronize(ctx->stream));
        P.g_lo = (T)l1; P.g_hi = (T)l2;
        desc.g_lambda = l1; desc.g_l2 = l2;
    }
    // ElasticNet's two numbers: finite and >= 0, in the problem's type too (an fp32 problem rounds them)
    static void enet_check(double l1, double l2) {
        const double big = (double)std::numeric_limits<T>::max();
        if (!(std::isfinite(l1) && l1 >= 0 && l1 <= big))
            throw Error(BZ_ERR_ARG, "ElasticNet: g_lambda (l1) must be finite and >= 0 in the problem's type");
        if (!(std::isfinite(l2) && l2 >= 0 && l2 <= big))
            throw Error(BZ_ERR_ARG, "ElasticNet: g_l2 (l2) must be finite and >= 0 in the problem's type");
    }
    const char* gname() const { return ragged_g ? "GroupLasso" : "NormL21"; }
    // ... of NormL21 and GroupLasso: a number for a number, a vector (one entry per group) for a vector; a refused call changes nothing
    void set_group_lambda(double lam, const void* lam_vec) {
        if (lam_vec && !P.group_lambda_vec())
            throw Error(BZ_ERR_ARG, std::string("bz_problem_set_g_lambda: the problem was created with a number lambda (") + gname() + " takes a vector at bz_problem_create only)");
        if (!lam_vec && P.group_lambda_vec())
            throw Error(BZ_ERR_ARG, std::string("bz_problem_set_g_lambda: the problem was created with a vector lambda of ") + gname() + ": pass a vector");
        std::vector<T> h;
        if (lam_vec) read_group_lambda_vec(lam_vec, h);
        else if (!(std::isfinite(lam) && lam >= 0)) throw Error(BZ_ERR_ARG, std::string(gname()) + ": lambda must be finite and >= 0");
        gate_abort();
        BZ_HIP(hipStreamSynchronize(ctx->stream));
        if (lam_vec) copy_in(glam_.p, h.data(), grp_ng_);
        else { P.g_lambda = (T)lam; desc.g_lambda = lam; }
    }
    // NormL21's and GroupLasso's per-group lambda on a host copy: one entry per group, finite and >= 0 (a zero: an unpenalised group)
    void read_group_lambda_vec(const void* src, std::vector<T>& h) {
        h.resize((size_t)(grp_ng_));
        BZ_HIP(hipMemcpy(h.data(), src, h.size() * sizeof(T), hipMemcpyDefault));
        for (size_t i = 0; i < h.size(); ++i)
            if (!(std::isfinite((double)h[i]) && h[i] >= T(0)))
                throw Error(BZ_ERR_ARG, std::string(gname()) + ": every entry of the vector lambda must be finite and >= 0 (entry " + std::to_string(i) + ")");
    }
    // NormL1's per-element lambda on a host copy: every entry finite and >= 0 (zeros are the unpenalised coefficients)
    void read_lambda_vec(const void* src, std::vector<T>& h) { read_elem_vec(src, h, "NormL1", "the vector lambda"); }
    // a per-element vector of g (NormL1's lambda, ElasticNet's penalty factors) on a host copy: nx entries, finite and >= 0
    void read_elem_vec(const void* src, std::vector<T>& h, const char* kind, const char* field) {
        h.resize((size_t)nx);
        BZ_HIP(hipMemcpy(h.data(), src, h.size() * sizeof(T), hipMemcpyDefault));
        for (int64_t i = 0; i < nx; ++i)
            if (!(std::isfinite((double)h[i]) && h[i] >= T(0)))
                throw Error(BZ_ERR_ARG, std::string(kind) + ": every entry of " + field + " must be finite and >= 0 (entry " + std::to_string(i) + ")");
    }

    void set_multipliers(const void* mu, const void* y) override {
        copy_in(mu_.p, mu, ny);
        copy_in(ymul_.p, y, ny);
        aug_lag_update();
    }

    void begin(const bz_panoc_opts& o, const void* x0_host) override {
        copy_in(X_[0].p, x0_host, n);
        begin_dev(o, X_[0].p);
    }

    void solve(const bz_panoc_opts& o, const void* x0, void* x_out, bz_panoc_stats* st) override {
        begin(o, x0);
        run_to_completion();
        finish(x_out, st);
    }

    bool should_stop() const override {
        return cnt_.k >= opt.maxit || (double)stop_norm_ <= opt.tol;
    }

    void finish(void* x_out, bz_panoc_stats* st) override {
        require_active();
        if (x_out) { ensure_z(false); copy_out(x_out, Z_[zc].p, n); }
        if (st) fill_stats(st);
    }

    void scalars(double* o) override {
        require_active();
        o[0] = (double)cnt_.k; o[1] = (double)state_.gamma; o[2] = (double)tau; o[3] = (double)state_.f_x;
        o[4] = (double)state_.g_z; o[5] = (double)state_.dot_gr; o[6] = (double)state_.ss_res; o[7] = stop_norm_;
        o[8] = (double)last_ys; o[9] = (double)state_.lbfgs.order.size(); o[10] = (double)state_.lbfgs.H;
        o[11] = (double)state_.f_z_al; o[12] = (double)state_.fraw_last; o[13] = (double)last_nbt;
        o[14] = last_fused ? 1.0 : 0.0; o[15] = (double)state_.fbe_last;
    }

    void vector(int which, void* out) override {
        require_active();
        switch (which) {
        case 0: copy_out(out, X_[xc].p, n); break;
        case 1: ensure_z(false); copy_out(out, Z_[zc].p, n); break;
        case 2: ensure_z(); copy_out(out, RES_[rc].p, n); break;
        case 3:
            if (!state_.gx_valid) { dense_redo([&] { algrad(X_[xc].p, GX_.p, SL_AUX); }); state_.gx_valid = true; }
            copy_out(out, GX_.p, n); break;
        case 4:
            ensure_z();
            if (!state_.gz_valid) { dense_redo([&] { algrad(Z_[zc].p, GZ_.p, SL_AUX); }); state_.gz_valid = true; }
            copy_out(out, GZ_.p, n); break;
        default: throw Error(BZ_ERR_ARG, "unknown vector id");
        }
    }

    void eval_al_gradient(const void* x, void* dlx, double* vals3) override {
        copy_in(TMP_.p, x, n);
        std::vector<double> v;
        dense_redo([&] {
            algrad(TMP_.p, D_.p, SL_AUX);           // (exchanges its two slots itself)
            v = collect({SL_AUX, SL_AUX + 1}, 0u);
        });
        T half_pen = T(0.5) * T(v[1]);
        vals3[0] = (double)al_value(v[0], v[1]);
        vals3[1] = (double)f_value(v[0]);
        vals3[2] = (double)half_pen;
        if (dlx) copy_out(dlx, D_.p, n);
    }

    void eval_prox(const void* x, double gam, void* z, double* gz) override {
        copy_in(TMP_.p, x, n);
        fbstep(TMP_.p, nullptr, (T)gam, D_.p, nullptr, SL_GSUM);
        gather(SL_GSUM, 3, 0u);
        auto v = collect({SL_GSUM}, 0u);
        *gz = (double)g_value(v[0]);
        copy_out(z, D_.p, n);
    }

    void eval_lbfgs(int m, const void* S, const void* Y, const void* v, void* d) override {
        if (m < 0 || m > MAX_MEM) throw Error(BZ_ERR_ARG, "bad pair count");
        active = false;
        state_.lbfgs.reset_all(std::max(1, m));
        alloc_history();
        rc = 0; xc = 0;
        const T* Sh = (const T*)S; const T* Yh = (const T*)Y;
        for (int i = 0; i < m; ++i) {   // oldest first, as update! would have seen them
            const int slot = state_.lbfgs.spare;
            copy_in(S_[slot].p, Sh + (size_t)i * n, n);
            copy_in(Y_[slot].p, Yh + (size_t)i * n, n);
            mv(2); launch(C_MISC, k_dot<T>, grid, (const T*)S_[slot].p, (const T*)Y_[slot].p, T(1), n, parts_.p, (int)SL_YS);
            mv(1); launch(C_MISC, k_dot<T>, grid, (const T*)Y_[slot].p, (const T*)Y_[slot].p, T(1), n, parts_.p, (int)SL_YTY);
            gather(SL_YS, 2, 0u);
            auto r = collect({SL_YS, SL_YTY}, 0u);
            state_.lbfgs.insert((T)r[0], (T)r[1], nullptr, nullptr, compact_ok, dir_kind_ == BZ_DIR_ANDERSON);
        }
        // d = H * v  == two-loop applied to -(-v)
        std::vector<T> neg(n);
        const T* vh = (const T*)v;
        for (int64_t i = 0; i < n; ++i) neg[i] = -vh[i];
        copy_in(RES_[rc].p, neg.data(), n);
        TailArgs<T> t = two_loop();
        mv(t.mode != 2 ? 3 : 2);
        launch(C_TWOLOOP, k_axpy_dot<T>, grid, t, (const T*)nullptr, (const T*)nullptr, D_.p, n,
               parts_.p, 0);
        copy_out(d, D_.p, n);
    }

    void profile_enable(unsigned mask) override {
        prof_mask = mask & 0xFFFFu;
        prof_period = std::max(1u, mask >> 16);          // upper 16 bits: time every k-th launch only
        for (auto& c : prof_count) c = 0;
    }
    void profile_reset() override {
        drain_prof();
        for (int c = 0; c < BZ_NUM_KERNEL_CATEGORIES; ++c) {
            prof_ms[c] = 0; prof_n[c] = 0; bytes_all_[c] = 0; bytes_timed_[c] = 0; launches_all_[c] = 0;
        }
    }
    void profile_get2(int cat, bz_profile_rec* r) override {
        if (cat < 0 || cat >= BZ_NUM_KERNEL_CATEGORIES) throw Error(BZ_ERR_ARG, "bad category");
        drain_prof();
        std::memset(r, 0, sizeof(*r));
        r->timed_launches = prof_n[cat]; r->timed_ms = prof_ms[cat]; r->timed_bytes = bytes_timed_[cat];
        r->launches = launches_all_[cat]; r->bytes = bytes_all_[cat];
        std::strncpy(r->form, form_[cat].c_str(), sizeof(r->form) - 1);
    }
    void profile_get(int cat, int64_t* launches, double* ms) override {
        if (cat < 0 || cat >= BZ_NUM_KERNEL_CATEGORIES) throw Error(BZ_ERR_ARG, "bad category");
        drain_prof();
        *launches = prof_n[cat];
        *ms = prof_ms[cat];
    }

    // ------------------------------------------------------- alps (alps.jl:7-117)
    void alps(const bz_alps_opts& ao, const bz_panoc_opts& po, const void* x0, const void* y0,
              void* xo, void* yo, void* so, void* muo, bz_alps_stats* st) override {
        if (slack) throw Error(BZ_ERR_STATE, "bz_alps_solve on a slack (ALS) problem: use bz_als_solve");
        if (ao.warm_start & ~1) throw Error(BZ_ERR_ARG, "bz_alps_opts.warm_start: unknown bit (bit 0: the step size)");
        auto t0 = std::chrono::steady_clock::now();
        const T epsT = std::numeric_limits<T>::epsilon();
        T* x = X_[0].p;
        copy_in(TMP_.p, x0, n);
        // prox!(x, gFun, x0, eps(T))                                   alps.jl:38
        fbstep(TMP_.p, nullptr, epsT, x, nullptr, SL_GSUM);
        gather(SL_GSUM, 3, 0u);
        // objx = f(x) + gFun.gz                                        alps.jl:39
        fvalue(x, SL_AUX);
        auto v0 = collect({SL_GSUM, SL_AUX}, 0u);
        T gz0 = g_value(v0[0]);
        T objx = f_value(v0[1]) + gz0;
        // eval!(cx,c,x); proj!(s,D,cx); default_penalty_parameter!     alps.jl:40-42
        const double denom = std::max(1.0, (double)objx);
        const bool dense_c = desc.c_kind == BZ_C_DENSE_AFFINE || desc.c_kind == BZ_C_SPARSE_AFFINE;      // c(x) lives in CX_
        if (dense_c) eval_c(x);
        if (generic_) {
            // eval!(cx, c, x) ; proj!(s, D, cx) ; default_penalty_parameter!   (alps.jl:40-42, safeguards.jl:13-18:
            // Float64 literals, stored back into T — the arithmetic of k_penalty_init)
            copy_out(hx_.data(), x, n);
            cb_c_eval(hx_.data(), hcx_.data(), n, ny);
            cb_D_proj(hcx_.data(), hs_.data(), ny);
            for (int64_t i = 0; i < ny; ++i) {
                const T dd = hcx_[i] - hs_[i];
                const double h = 0.5 * (double)(dd * dd);
                T mm = (T)(((h > 1.0 || h != h) ? h : 1.0) / denom);      // (a NaN distance stays NaN, as in k_penalty_init)
                mm = (T)((double)mm * 0.1);
                double w = (double)mm;
                w = (w < 1e8 || w != w) ? w : 1e8;
                w = (w > 1e-8 || w != w) ? w : 1e-8;
                hmu_[i] = (T)w;
            }
            copy_in(sproj_.p, hs_.data(), ny);
            copy_in(mu_.p, hmu_.data(), ny);
        } else {
        mv(3 + (P.D_lo_vec ? 1 : 0) + (P.D_hi_vec ? 1 : 0), ny);
        launch(C_MISC, k_penalty_init<T>, grid_y, dense_c ? (const T*)CX_.p : (const T*)x /* cx = x */, P, denom,
               sproj_.p, mu_.p, ny);
        }
        copy_in(ymul_.p, y0, ny);                                    // y .= y0
        double norm_res_prim = 0, norm_res_prim_old = 0;
        bool have_old = false, have_res = false;
        int64_t tot_it = 0, tot_inner = 0;
        double inner_tol = ao.inner_tol;
        bool solved = false, tired = tot_it >= ao.maxit, broken = std::isnan((double)objx);
        if (ao.verbose) {
            std::printf("[ Info: initial inner tolerance %g\n", inner_tol);
        }
        bool can_stop = solved || tired || broken;
        bz_panoc_opts po2 = po;
        while (!can_stop) {
            ++tot_it;
            po2.tol = inner_tol;                                     // alps.jl:64
            po2.verbose = ao.verbose;
            // opt-in (bz_alps_opts.warm_start bit 0): subsolver(tol, verbose; gamma = gamma_prev, adaptive = true)
            if ((ao.warm_start & 1) && tot_it > 1 && (double)state_.gamma > 0.0) { po2.gamma = (double)state_.gamma; po2.adaptive = 1; }
            // dual_safeguard(y, cx)  alps.jl:62  +  AugLagUpdate!  alps.jl:65, one pass
            aug_lag_update(true);
            begin_dev(po2, x);                                       // alps.jl:66
            run_to_completion();
            const int64_t sub_it = cnt_.k;
            ensure_z(false);
            x = Z_[zc].p;                                            // x .= sub_sol
            objx = state_.fraw_last + state_.g_z;                    // alps.jl:68
            tot_inner += sub_it;
            const bool sub_solved = sub_it < ao.subsolver_maxit;     // alps.jl:70
            // dual update + primal residual                          alps.jl:72-84
            if (dense_c) eval_c(x);                                  // eval!(cx, c, x)  alps.jl:72
            if (generic_) {
                copy_out(hx_.data(), x, n);
                cb_c_eval(hx_.data(), hcx_.data(), n, ny);          // eval!(cx, c, x)      alps.jl:72
                for (int64_t i = 0; i < ny; ++i) hyv_[i] = hcx_[i] + hmuy_[i];         // y .= cx .+ muy       :74
                cb_D_proj(hyv_.data(), hs_.data(), ny);             // proj!(s, D, y)       :75
                double nrm = 0.0;
                for (int64_t i = 0; i < ny; ++i) {
                    T t = hyv_[i] - hs_[i];                                            // y .-= s              :80
                    hyv_[i] = t / hmu_[i];                                             // y ./= mu             :81
                    const T r = hcx_[i] - hs_[i];
                    const double ar = (double)(r < T(0) ? -r : r);
                    if (ar > nrm || ar != ar) nrm = ar;                                // norm(cx - s, Inf)    :84
                }
                copy_in(ymul_.p, hyv_.data(), ny);
                copy_in(sproj_.p, hs_.data(), ny);
                fill_slot(SL_OUTER, nrm);
            } else {
            mv(3 + pstreams(false, true, false), ny);
            launch(C_MISC, k_dual_update<T>, grid_y, dense_c ? (const T*)CX_.p : (const T*)x, P, ymul_.p, sproj_.p,
                   ny, parts_.p, (int)SL_OUTER);
            }
            gather(SL_OUTER, 1, 1u, 1u);
            auto r = collect({SL_OUTER}, 1u);
            norm_res_prim_old = norm_res_prim; have_old = have_res;
            norm_res_prim = r[0]; have_res = true;
            solved = (inner_tol <= ao.tol_dual && sub_solved) && (norm_res_prim <= ao.tol_prim);
            tired = tot_it >= ao.maxit;
            broken = std::isnan((double)objx);
            can_stop = solved || tired || broken;
            if (!can_stop) {
                if (have_old &&
                    norm_res_prim > std::max(ao.theta_penalty * norm_res_prim_old, ao.tol_prim)) {
                    mv(2, ny); launch(C_MISC, k_clamp_scale<T>, grid_y, mu_.p, 0.0, 0.0, (T)ao.kappa_penalty, 0, ny);
                }
                inner_tol = std::max(ao.kappa_tol * inner_tol, ao.tol_dual);
            }
            // next subproblem starts from x (kept in the z buffer): copy to a state buffer
            // (the z buffer BECOMES the first state buffer: the next bz_panoc_begin recomputes z anyway)
            if (!can_stop) {
                X_[0].swap(Z_[zc]);
                x = X_[0].p;
            }
        }
        copy_out(xo, x, n);
        copy_out(yo, ymul_.p, ny);
        copy_out(so, sproj_.p, ny);
        copy_out(muo, mu_.p, ny);
        if (st) {
            st->tot_it = tot_it; st->tot_inner_it = tot_inner;
            st->elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            st->status = solved ? 0 : (tired ? 1 : (broken ? 2 : 3));
            st->inner_tol = inner_tol; st->norm_res_prim = norm_res_prim;
            st->objective = (double)objx;
        }
    }

    // ------------------------------------------------------- als (als.jl:7-120)
    void als(const bz_alps_opts& ao, const bz_panoc_opts& po, const void* x0, const void* y0,
             void* xo, void* yo, void* so, void* muo, bz_alps_stats* st) override {
        if (!slack) throw Error(BZ_ERR_STATE, "bz_als_solve needs a problem created with desc.slack = 1");
        if (ao.warm_start & ~1) throw Error(BZ_ERR_ARG, "bz_alps_opts.warm_start: unknown bit (bit 0: the step size)");
        auto t0 = std::chrono::steady_clock::now();
        const T epsT = std::numeric_limits<T>::epsilon();
        T* xs = X_[0].p;                                   // [x; s]
        copy_in(TMP_.p, x0, nx);
        // prox!(x, gFun, x0, eps(T)) ; objx = f(x) + gFun.gz              als.jl:41-42
        mv(2 + pstreams(false, false, true), nx);
        if (lp_g) launch(C_FB, k_fbstep<T, true>, grid_x, (const T*)TMP_.p, (const T*)nullptr, epsT, P, xs, (T*)nullptr, nx, parts_.p, (int)SL_GSUM);
        else launch(C_FB, k_fbstep<T, false>, grid_x, (const T*)TMP_.p, (const T*)nullptr, epsT, P, xs, (T*)nullptr, nx, parts_.p, (int)SL_GSUM);
        for (int k = 0; k < 3; ++k) slot_n[SL_GSUM + k] = grid_x;
        fvalue(xs, SL_AUX);
        auto v0 = collect({SL_GSUM, SL_AUX}, 0u);
        T objx = f_value(v0[1]) + g_value(v0[0]);
        // eval!(cx,c,x); proj!(s,D,cx); default_penalty_parameter!          als.jl:43-45   (s lands in xs[nx:])
        if (slack_dense) eval_c(xs);                                 // cx = A x - b -> CX_ ; c = Identity: cx is x itself
        mv(3 + (P.D_lo_vec ? 1 : 0) + (P.D_hi_vec ? 1 : 0), ny);
        launch(C_MISC, k_penalty_init<T>, grid_y, slack_dense ? (const T*)CX_.p : (const T*)xs, P, std::max(1.0, (double)objx),
               xs + nx, mu_.p, ny);
        copy_in(ymul_.p, y0, ny);
        double norm_res_prim = 0, norm_res_prim_old = 0;
        bool have_old = false, have_res = false;
        int64_t tot_it = 0, tot_inner = 0;
        double inner_tol = ao.inner_tol;
        bool solved = false, tired = tot_it >= ao.maxit, broken = std::isnan((double)objx);
        if (ao.verbose) std::printf("[ Info: initial inner tolerance %g\n", inner_tol);
        bool can_stop = solved || tired || broken;
        bz_panoc_opts po2 = po;
        while (!can_stop) {
            ++tot_it;
            po2.tol = inner_tol; po2.verbose = ao.verbose;
            if ((ao.warm_start & 1) && tot_it > 1 && (double)state_.gamma > 0.0) { po2.gamma = (double)state_.gamma; po2.adaptive = 1; }
            aug_lag_update(true);                                    // dual_safeguard + AugLagUpdate!(fSlack, mu, y)
            begin_dev(po2, xs);                                      // sub_solver(f=fSlack, g=gSlack, x0=xSlack)
            run_to_completion();
            const int64_t sub_it = cnt_.k;
            ensure_z(false);                                         // (the one-pass kernel keeps z in registers until it is asked for)
            xs = Z_[zc].p;                                           // xSlack .= sub_sol
            objx = state_.fraw_last + state_.g_z;                    // f(x) + gSlack.gz       als.jl:79
            tot_inner += sub_it;
            const bool sub_solved = sub_it < ao.subsolver_maxit;
            // y += (cx - s)/mu ; ||cx - s||_inf                      als.jl:82-87
            if (slack_dense) {
                eval_c(xs);                                          // eval!(cx, c, x) at the subsolver's solution   als.jl:82
                mv(5, ny); nm("k_dual_update_slack_rows");
                launch(C_MISC, k_dual_update_slack_rows<T>, grid_y, (const T*)CX_.p, (const T*)(xs + nx), (const T*)mu_.p,
                       ymul_.p, ny, parts_.p, (int)SL_OUTER);
            } else {
                mv(5, nx);
                launch(C_MISC, k_dual_update_slack<T>, grid_y, (const T*)xs, (const T*)mu_.p, ymul_.p, nx, parts_.p,
                       (int)SL_OUTER);
            }
            slot_n[SL_OUTER] = grid_y;
            gather(SL_OUTER, 1, 1u);
            auto r = collect({SL_OUTER}, 1u);
            norm_res_prim_old = norm_res_prim; have_old = have_res;
            norm_res_prim = r[0]; have_res = true;
            solved = (inner_tol <= ao.tol_dual && sub_solved) && (norm_res_prim <= ao.tol_prim);
            tired = tot_it >= ao.maxit;
            broken = std::isnan((double)objx);
            can_stop = solved || tired || broken;
            if (!can_stop) {
                if (have_old && norm_res_prim > std::max(ao.theta_penalty * norm_res_prim_old, ao.tol_prim)) {
                    mv(2, ny); launch(C_MISC, k_clamp_scale<T>, grid_y, mu_.p, 0.0, 0.0, (T)ao.kappa_penalty, 0, ny);
                }
                inner_tol = std::max(ao.kappa_tol * inner_tol, ao.tol_dual);
                BZ_HIP(hipMemcpyAsync(X_[0].p, xs, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
                xs = X_[0].p;
            }
        }
        copy_out(xo, xs, nx);
        copy_out(so, xs + nx, ny);
        copy_out(yo, ymul_.p, ny);
        copy_out(muo, mu_.p, ny);
        if (st) {
            st->tot_it = tot_it; st->tot_inner_it = tot_inner;
            st->elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            st->status = solved ? 0 : (tired ? 1 : (broken ? 2 : 3));
            st->inner_tol = inner_tol; st->norm_res_prim = norm_res_prim;
            st->objective = (double)objx;
        }
    }

   private:
    // ------------------------------------------------------------ plumbing
    Ctx* ctx;
    bz_problem_desc desc;
    int64_t n, ny;
    int64_t nx;                              // length of x (== n unless slack: then n = nx + ny)
    bool slack;
    const CreateKnobs cenv_;                 // the knobs read when the problem was created
    BeginKnobs env_;                         // ... at the last bz_panoc_begin (at creation before the first)
    int grid = 1, grid_y = 1;
    int grid_x = 1;                          // kernels over x alone (== grid unless slack)
    bool slack_dense = false;                // slack form with c = DenseAffine: halves of unequal length
    int lgx_ = 1, lgs_ = 1;                  // k_fbstep_lifted: workgroups of its x section and of its s section
    // the sections of a launch over the lifted vector: a function of (nx, ny) alone, so that the partial sums are too
    static void lifted_sections(int64_t nx_, int64_t ny_, int& gx, int& gs) {
        constexpr int64_t N = PackN<T>::N;
        gx = (int)std::min<int64_t>(PSTRIDE / 2, std::max<int64_t>(1, ((nx_ + N - 1) / N + BLOCK - 1) / BLOCK));
        gs = (int)std::min<int64_t>(PSTRIDE / 2, std::max<int64_t>(1, ((ny_ + N - 1) / N + BLOCK - 1) / BLOCK));
    }
    ElemParams<T> P;
    DBuf<T> q_, b_, gu_, glam_, glo_, ghi_, dlo_, dhi_, mu_, muy_, ymul_, sproj_;
    // x lives in a ring long enough to keep the last CM+1 iterates alive (history as iterates, see xr_run_): CM+1
    // snapshots + the slot being written (+ one more slot for the tau blend); res in two slots, the current and the next
    static constexpr int NXR = CM + 3, NRR = 2;
    DBuf<T> X_[NXR], RES_[NRR], Z_[2], GX_, GZ_, D_, TMP_;
    DBuf<T> A_, cb_, CX_, YU_, GT_;          // DenseAffine c: A[ny][n], b, c(x), yupd, A'v row-chunk partials
    int rows_per_chunk = 1, nrowchunks = 1;
    DBuf<T> FA_, fb_, FR_, DFX_, FGT_;       // dense f: matrix, vector, residual / Qx, gradient of f, A_f'r row-chunk partials
    bool dense_f = false, sparse_f = false, lp_g = false;      // (sparse_f: the sparse quadratic; sparse_ls: at the end)
    bool group_g = false;                    // g = NormL21 or GroupLasso: kept on the kernel chain wherever lp_g is; k_fbstep_group / k_fbstep_ragged its one kernel
    int grp_K_ = 0, grp_KP_ = 0;             // ... its group size K and the power of two >= K
    int64_t grp_ng_ = 0;                     // ... the number of groups (of both group kinds)
    bool enet_g = false;                     // g = ElasticNet: an element-wise run-time kind, no one-pass family, no fast slack form
    bool ragged_g = false;                   // g = GroupLasso (a group pointer; group_g holds too): k_fbstep_ragged its one kernel
    std::vector<int64_t> grp_ptr_h_;         // ... ptr[ng + 1] on the host, validated
    DBuf<int64_t> gptr_;                     // ... and on the device
    int grp_L_ = 1;                          // ... lanes per group (ragged_lanes: from the mean size)
    int64_t grp_max_ = 0, grp_swept_ = 0;    // ... the longest group; the elements in waves that sweep twice
    // generic oracles (host callbacks): host mirrors of the vectors the callbacks read and write
    bool generic_ = false;
    std::vector<T> hx_, hg_, hy_, hz_, hres_, hdfx_, hjtv_, hcx_, ht_, hs_, hmu_, hmuy_, hyv_;
    // the five host callbacks; a callback that failed says so through bz_callback_abort() (it cannot unwind through the
    // C frames): the library call in progress then ends with BZ_ERR_CALLBACK as soon as the callback has returned,
    // instead of iterating on whatever the failed callback left in its output buffers
    static void cb_check() {
        if (callback_abort_flag()) { callback_abort_flag() = false; throw Error(BZ_ERR_CALLBACK, "an oracle callback failed (bz_callback_abort)"); }
    }
    void cb_c_eval(const T* x, T* cx, int64_t n_, int64_t ny_) { desc.cb_c_eval(desc.cb_user, x, cx, n_, ny_); cb_check(); }
    void cb_D_proj(const T* v, T* s, int64_t ny_) { desc.cb_D_proj(desc.cb_user, v, s, ny_); cb_check(); }
    void cb_c_jtprod(const T* x, const T* v, T* jtv, int64_t n_, int64_t ny_) { desc.cb_c_jtprod(desc.cb_user, x, v, jtv, n_, ny_); cb_check(); }
    double cb_f_gradient(const T* x, T* dfx, int64_t n_) { const double v = desc.cb_f_gradient(desc.cb_user, x, dfx, n_); cb_check(); return v; }
    double cb_g_prox(const T* x, double gam, T* z, int64_t n_) { const double v = desc.cb_g_prox(desc.cb_user, x, gam, z, n_); cb_check(); return v; }
    void fill_slot(int slot, double v) {
        launch_b(C_MISC, k_fill_slot, 1, 64, parts_.p, slot, v);
        slot_n[slot] = 1;
    }
    // gradient!(dlx, al, x) with the oracles evaluated on the host, statement by statement as
    // src/utilities/auglagfun.jl:73-86 (the value-only form :58-69 is the same minus dfx and jtv)
    void algrad_generic(const T* x, T* grad, int slot0) {
        copy_out(hx_.data(), x, n);
        cb_c_eval(hx_.data(), hcx_.data(), n, ny);                  // eval!(cx, c, x)          :74
        for (int64_t i = 0; i < ny; ++i) ht_[i] = hcx_[i] + hmuy_[i];                  // yupd .= cx .+ muy        :75
        cb_D_proj(ht_.data(), hs_.data(), ny);                      // proj!(s, D, yupd)        :76
        double pen = 0.0;
        for (int64_t i = 0; i < ny; ++i) {
            T t = ht_[i] - hs_[i];                                                     // yupd .-= s               :77
            pen += (double)((t * t) / hmu_[i]);                                        // sum(yupd.^2 ./ mu)       :78
            ht_[i] = t / hmu_[i];                                                      // yupd ./= mu              :79
        }
        const double fx = cb_f_gradient(hx_.data(), hdfx_.data(), n);   // fx = gradient!(dfx, f, x)  :80
        if (grad) {
            cb_c_jtprod(hx_.data(), ht_.data(), hjtv_.data(), n, ny);   // jtprod!(jtv, c, x, yupd)   :83
            for (int64_t j = 0; j < n; ++j) hg_[j] = hdfx_[j] + hjtv_[j];              // dlx .= dfx .+ jtv        :84
            copy_in(grad, hg_.data(), n);
        }
        fill_slot(slot0, fx);
        fill_slot(slot0 + 1, pen);
    }
    // y = x - gamma g ; z = prox!(., g, y, gamma) ; res = x - z   (nonsmoothcostfun.jl:17-22 and the caller's
    // forward step), with the sums k_fbstep returns
    void fbstep_generic(const T* x, const T* g, T gam, T* z, T* res, int slot0) {
        copy_out(hx_.data(), x, n);
        if (g) copy_out(hg_.data(), g, n);
        for (int64_t j = 0; j < n; ++j) {
            T yv = hx_[j];
            if (g) { T t = gam * hg_[j]; yv = hx_[j] - t; }
            hy_[j] = yv;
        }
        const double gz = cb_g_prox(hy_.data(), (double)gam, hz_.data(), n);
        double dot = 0.0, ss = 0.0;
        for (int64_t j = 0; j < n; ++j) {
            const T r = hx_[j] - hz_[j];
            hres_[j] = r;
            if (g) dot += (double)(hg_[j] * r);
            ss += (double)(r * r);
        }
        copy_in(z, hz_.data(), n);
        if (res) copy_in(res, hres_.data(), n);
        fill_slot(slot0, gz);
        fill_slot(slot0 + 1, dot);
        fill_slot(slot0 + 2, ss);
    }
    int64_t frows = 0, npad = 0, npadx = 0;
    int f_rows_per_chunk = 1, f_nrowchunks = 1;
    T fscale = T(1);                         // f(x) = fscale * (sum of the f partials)
    // persistent two-loop
    DBuf<unsigned long long> pcounter_, pgflag_;
    DBuf<double> pglobal_;                   // [0..1] phase totals (double-buffered), [2] final <y_0,d>
    int pblocks = 0;                         // blocks of the persistent grid (= CUs unless overridden)
    unsigned long long pbase = 0;
    int* ptimeout_ = nullptr;                // host-mapped
    int* ptimeout_dev_ = nullptr;
    int num_cus = 0, persist_kr = 0;
    int64_t vcap = 0;                        // allocated elements per n-vector (>= n, zero-padded)
    bool persist_ok = false;
    bool stencil_fast_ = false;              // Stencil5pt f with the two fused stencil passes (see step())
    // Affine images (dense affine c, D = ZeroSet / FreeSet, f = Zero / DiagQuadratic: c(.) and grad L(.) are affine maps):
    // the images of the trial point x + d are formed from the stored images of the iterates — the same linear
    // combination that forms d — instead of two passes over A; a pass-over-A evaluation every `aff_refresh_`
    // iterations stops rounding drift.  State: c and grad L at the current x and z (CXS_, GX_, CZS_, GZ_), their
    // candidates (CXD_, CZN_, GXN_, GZN_) and the images of every stored pair (AS_, AY_: ny-vectors; GS_, GY_: n).
    bool affine_ok_ = false, aff_track_ = false;
    int aff_refresh_ = 8;
    T* cx_keep_ = nullptr;                   // algrad (dense c): also leave c(point) here
    DBuf<T> CXS_, CZS_, CXD_, CZN_, GXN_, GZN_;
    std::vector<DBuf<T>> AS_, AY_, GS_, GY_;
    CompactVecs<T, CM> image_vecs(bool ny_space) const {      // logical (oldest first) view, as compact_vecs()
        CompactVecs<T, CM> V;
        std::memset(&V, 0, sizeof(V));
        V.m = (int)state_.lbfgs.order.size();
        for (int i = 0; i < V.m; ++i) {
            const int s = state_.lbfgs.order[V.m - 1 - i];
            V.S[i] = ny_space ? AS_[s].p : GS_[s].p;
            V.Y[i] = ny_space ? AY_[s].p : GY_[s].p;
        }
        return V;
    }
    bool persist_broken_ = false;            // a grid barrier timed out once on this problem: the kernel chain from then on
    int64_t n_persist_fallbacks_ = 0;
    std::vector<DBuf<T>> S_, Y_;
    DBuf<double> parts_, alphas_, send_, recv_;
    double* host_out_ = nullptr;             // pinned mailbox: {value, ticket} per collected scalar
    double* host_out_dev_ = nullptr;
    unsigned long long collect_seq = 0;
    int grp_first[SL_COUNT], grp_cnt[SL_COUNT];
    int slot_n[SL_COUNT];                    // number of valid block partials per slot

    // solver state (host scalars)
    bz_panoc_opts opt{};
    bool active = false, fused_ok = false;
    // History as iterates: once the last iterations were plain ones that each inserted their pair, the stored
    // pairs are the successive differences of the last iterates, which the long x ring still holds, and the
    // residual of an iterate is a function of that iterate alone (res = x - prox(x - gamma grad L(x)), with
    // gamma, mu, mu*y fixed along the run).  The fused pass then reads those iterates instead of S and Y,
    // re-evaluates their residuals instead of reading them, and re-forms the pairs by the very subtractions
    // that made them (s = x_d - x, y = res - res_prev): the same bits.  It stops WRITING s, y and res: reads
    // the iterates + q, b, mu, mu*y, writes x_d.  The first iteration that is not a plain one turns the
    // iterates back into pairs (k_pairs_from_iterates) and the classic kernels take over.
    int xr_run_ = 0;             // consecutive plain, pair-inserting iterations so far
    bool sy_stale_ = false;      // S_/Y_ do not hold the stored pairs (they live in the x ring)
    double gring_[NXR] = {0};    // the gamma the residual of each iterate in the ring was (or would be) formed with
    void materialize_pairs() { materialize_pairs((double)state_.gamma); }
    // gam_cur: the gamma the current iterate's residual is formed with (state_.gamma, but for a state whose last trial halved it)
    void materialize_pairs(double gam_cur) {
        if (!sy_stale_) return;
        SnapVecs<T, CM> V;
        std::memset(&V, 0, sizeof(V));
        const int m = (int)state_.lbfgs.order.size();      // (< CM soon after a memory reset)
        for (int i = 0; i <= CM; ++i) {
            const int back = std::max(0, m - i);
            V.XH[i] = X_[(xc - back + NXR) % NXR].p;
            V.gam[i] = back ? gring_[(xc - back + NXR) % NXR] : gam_cur;
        }
        for (int i = 0; i < m; ++i) { V.S[i] = S_[state_.lbfgs.order[m - 1 - i]].p; V.Y[i] = Y_[state_.lbfgs.order[m - 1 - i]].p; }
        if (slack) {
            // (the lifted vector: both halves of every iterate in, both halves of the pairs, the residual and z out)
            mv(2 * ((m + 1) + 2 * m + 2) + pstreams(true, true, true) + (P.uni >= 2 ? 0 : 1), nx);
            launch(C_MISC, k_pairs_from_iterates_slack<T, CM>, grid_y, V, m, P, (const T*)ymul_.p, RES_[rc].p, Z_[zc].p, nx);
        } else {
            // (must run before gamma changes: the residuals are re-evaluated with the gamma of this run)
            mv((m + 1) + pstreams(true, true, true) + 2 * m + 2);
            launch(C_MISC, k_pairs_from_iterates<T, CM>, grid, V, m, P, RES_[rc].p, Z_[zc].p, n);
        }
        state_.res_valid = true; state_.z_valid = true;
        sy_stale_ = false;
    }
    int xc = 0, rc = 0, zc = 0;
    T alpha = T(0.95), beta = T(0.5), min_gamma = T(1e-7), musqy = T(0);
    T gamma_given_ = T(0);       // bz_panoc_opts.gamma / alpha / Lf (0: estimate a Lipschitz constant)
    bool adaptive_ = true;       // upstream's `adaptive`: gamma halvings at the start and inside the line search
    T tau = T(0), last_ys = T(0);
    double stop_norm_ = 0;
    // What step_impl may change before its last read-back (the ring indices, the pair insertion and the stop norm are
    // committed after it): the state's scalars, the L-BFGS bookkeeping (a halving resets it), the image counters, the
    // validity flags, and which allocation each affine-image buffer holds — traded by pointer, and only the candidates
    // (GXN_, GZN_, CXD_, CZN_) and the spare pair's images are written.  step() snapshots this struct by copy and puts it
    // back by assignment: a member an iteration changes before its last read-back belongs here, and is then restored.
    struct ImageRef { T* p; size_t n; };
    struct IterState {
        T gamma = T(0), f_x = T(0), g_z = T(0), dot_gr = T(0), ss_res = T(0);
        T f_z_al = T(0), fraw_last = T(0), fbe_last = T(0);
        LbfgsMemory<T> lbfgs;
        int aff_count = 0;
        bool gx_valid = false, gz_valid = false;
        // The one-pass compact kernel computes z in registers and does not store it: nothing in a plain iteration
        // reads it back (the next iterate is x_d, the stopping test uses grad L(z) formed in the same pass), and
        // the store is the dearest of the kernel's streams (-8 % of its time).  Who does need it — a tau backtrack
        // (z_curr), the caller asking for the solution — gets it re-materialised bit for bit from x and gamma.
        bool z_valid = true;
        bool res_valid = true;       // RES_[rc] holds the residual of the current state
        int64_t n_affine = 0, n_affine_verify = 0, n_affine_blends = 0;
        ImageRef img[8] = {};        // image_bufs() as snapshot() found them (the DBufs own the memory; unused in state_ itself)
    };
    IterState state_;
    // the counters an iteration advances: every recovery in step() puts them back
    struct IterCounters { int64_t k = 0, n_grad = 0, n_prox = 0, n_bt = 0, n_halv = 0, n_fused = 0, n_skips = 0; };
    IterCounters cnt_;
    int last_nbt = 0;
    bool last_fused = false;
    std::chrono::steady_clock::time_point t_begin;
    // `directions` other than L-BFGS (bz_panoc_opts.directions)
    int dir_kind_ = BZ_DIR_LBFGS;
    T broyden_theta_bar_ = T(0.2);
    DBuf<T> HB_, BHy_, BsH_;                 // Broyden: the dense operator (n x n, row-major), H y, H's
    int b_rpc_ = 1, b_nch_ = 1;
    // Broyden: D_ = H res (the caller forms x_d = x - D_ through the returned tail)
    TailArgs<T> broyden_dir() {
        gemv_rows(HB_.p, n, n, RES_[rc].p, (const T*)nullptr, D_.p);
        TailArgs<T> t;
        std::memset(&t, 0, sizeof(t));
        t.alphas = alphas_.p;
        t.in = D_.p; t.v = nullptr; t.sgn = T(-1); t.mode = 2; t.apply_H = 0; t.H = T(1);
        t.src = ScalarSrc{parts_.p, 0, 1}; t.ys = T(1);
        return t;
    }
    void broyden_reset() {
        launch(C_MISC, k_set_identity<T>, (int)std::min<int64_t>(PSTRIDE, (n * n + BLOCK - 1) / BLOCK), HB_.p, n);
    }
    // update!(H, s, y) — the pair sits in S_[spare], Y_[spare]:
    //   Hy = H y ; sH = s'H ; delta = <Hy, s> / <s, s> ; theta = 1 if |delta| >= theta_bar else
    //   (1 - sgn(delta) theta_bar) / (1 - delta), sgn(0) = 1 ; H += (s - Hy) / <s, (1/theta - 1) s + Hy> * sH
    void broyden_update() {
        const T* sv = S_[state_.lbfgs.spare].p;
        const T* yv = Y_[state_.lbfgs.spare].p;
        gemv_rows(HB_.p, n, n, yv, (const T*)nullptr, BHy_.p);
        gemv_cols(HB_.p, n, n, sv, b_rpc_, b_nch_, GT_.p, npad);
        {
            ElemParams<T> Pz = P;
            Pz.f_kind = BZ_F_ZERO;
            launch(C_MISC, k_gemv_t_finish<T>, grid, (const T*)GT_.p, b_nch_, npad, sv, Pz, BsH_.p, n, parts_.p, (int)SL_SCRATCH);
        }
        launch(C_MISC, k_dot<T>, grid, (const T*)BHy_.p, sv, T(1), n, parts_.p, (int)SL_AUX);
        launch(C_MISC, k_dot<T>, grid, sv, sv, T(1), n, parts_.p, (int)SL_AUX + 1);
        slot_n[SL_AUX] = slot_n[SL_AUX + 1] = grid;
        gather(SL_AUX, 2, 0u);
        auto v = collect({SL_AUX, SL_AUX + 1}, 0u);
        const T hys = T(v[0]), ss = T(v[1]);
        if (!(ss > T(0))) return;
        const T delta = hys / ss;
        T theta = T(1);
        if (std::abs(delta) < broyden_theta_bar_) {
            const T sg = delta >= T(0) ? T(1) : T(-1);
            theta = (T(1) - sg * broyden_theta_bar_) / (T(1) - delta);
        }
        const T denom = (T(1) / theta - T(1)) * ss + hys;
        if (denom == T(0) || denom != denom) return;
        launch(C_MISC, k_rank1_update<T>, (int)std::min<int64_t>(PSTRIDE, (n * n + BLOCK - 1) / BLOCK), HB_.p, sv,
               (const T*)BHy_.p, (const T*)BsH_.p, T(1) / denom, n);
    }
    bool compact_ok = false;                 // the compact form of the memory serves this solve (select_paths)

    // ---- gated pre-launch of the next iteration's one-pass kernel (see GateRec in bz_kernels.h) ----
    struct GatePlan {                        // everything the launch needs except the coefficients and the z address
        const T* S[CM];
        const T* x;
        T* xd;
        double gam0, gamma;
        int uni, gfc, fam, m_now;
        bool nt, table, keep_params, lds_ring;
        auto key() const { return std::tie(x, xd, gam0, gamma, uni, gfc, fam, m_now, nt, table, keep_params, lds_ring); }
        bool operator==(const GatePlan& o) const { return std::equal(S, S + CM, o.S) && key() == o.key(); }
    };
    // The headline pass's invariant parameter streams q and b through the Infinity Cache (k_fused_compact<..., PP = 1>:
    // default-policy loads for them, non-temporal for the ring and x_d) while both fit it.  Bare 6-iterate + q + b + x_d
    // pass, one workgroup per CU (tools/probes/mall_params.hip): n = 1e7 122.3 -> 100.7 us, 1.3e7 158.6 -> 129.7,
    // 1.6e7 200.9 -> 159.6 (q + b = 256 MB); with q and b on four rotating copies (never resident) no gain at any n.
    static constexpr double KEEP_PARAMS_BYTES = 256e6;
    bool keep_params(bool nt, bool table, int fam) const {
        if (!nt || table || fam != FAM_HEADLINE) return false;
        return env_.keepp >= 0 ? env_.keepp != 0 : (double)n * sizeof(T) * 2 <= KEEP_PARAMS_BYTES;
    }
    // The non-temporal headline pass (fp64) loads its packs ahead into a per-wave LDS ring instead of two register stages
    // (k_fused_compact<..., LQ = 1>): the LDS read one pack ahead of use, 246 VGPRs instead of 256 + 18 AGPRs.
    bool lds_ring(bool nt, bool table) const { return sizeof(T) == 8 && nt && !table && env_.ldsq != 0; }
    GateRec* gate_host_ = nullptr;           // pinned host memory
    GateRec* gate_host_dev_ = nullptr;       // ... its device address
    DBuf<GateRec> gate_dev_;
    unsigned long long gate_seq_ = 0;
    bool gate_pending_ = false, more_coming_ = false;
    int gate_env_ = 1;
    bool gate_broken_ = false;
    int gate_sabotage_ = 0;                  // (test) the n-th release is withheld: the launch must time out at its gate
    int64_t n_gate_fallbacks_ = 0;
    GatePlan gate_plan_{};
    double gate_bytes_ = 0.0;
    int64_t n_gated_ = 0, n_gate_aborts_ = 0;
    void gate_alloc() {
        if (gate_host_) return;
        BZ_HIP(hipHostMalloc((void**)&gate_host_, sizeof(GateRec), hipHostMallocMapped));
        std::memset(gate_host_, 0, sizeof(GateRec));
        BZ_HIP(hipHostGetDevicePointer((void**)&gate_host_dev_, gate_host_, 0));
        gate_dev_.alloc(1);
    }
    // (per-stream offsets of the one-pass kernels in 32 bits while every vector is shorter than 4 GB)
    bool small_vectors() const { return (double)vcap * sizeof(T) < 4.0e9; }
    // streams of the iterate-history pass without z: the m_now + 1 distinct iterates (x among them), the family's parameter
    // vectors (mu / mu*y unless passed as numbers), x_d
    int xr2_streams(int m_now) const { return (m_now + 1) + pstreams(true, true, true) + 1; }
    // The plan of the iterate-history pass (k_fused_compact<XR=2>) at ring position xc_ with m_now stored pairs, the ring's
    // gammas gring, a run of xr_run pairs that are ring differences, and z stored or not (false: that form does not apply).
    // The step plans the pass it runs here and the gated pre-launch plans the next iteration's: a pre-launched pass is
    // released only if the two plans are equal.
    bool xr2_plan(int xc_, int m_now, const double* gring, int xr_run, bool zstore, GatePlan& pl) const {
        const int fam = fused_family();
        if (!(env_.xr && small_vectors() && fam >= 0 && xr_run >= m_now)) return false;
        // (only the oldest stored iterate may carry another gamma — see CompactCoef::gam0)
        for (int i = 1; i < m_now; ++i)
            if (gring[(xc_ - m_now + i + NXR) % NXR] != (double)state_.gamma) return false;
        std::memset(&pl, 0, sizeof(pl));
        for (int i = 0; i < CM; ++i) {
            const int slot = (xc_ - std::max(0, m_now - i) + NXR) % NXR;      // (beyond m: x itself)
            pl.S[i] = X_[slot].p;
            if (i == 0) pl.gam0 = gring[slot];
        }
        pl.x = X_[xc_].p; pl.xd = X_[(xc_ + 1) % NXR].p;
        pl.gamma = (double)state_.gamma; pl.uni = uni_; pl.fam = fam; pl.m_now = m_now;
        // (one wave per SIMD, see trial_onepass)
        pl.gfc = env_.gfc > 0 ? std::min(grid, env_.gfc * std::max(1, num_cus)) : std::min(grid, std::max(1, num_cus));
        pl.nt = env_.nt >= 0 ? env_.nt != 0 : (double)n * sizeof(T) * (xr2_streams(m_now) + (zstore ? 1 : 0)) > 340e6;
        // (the headline family with everything uniform fixed at compile time, see the kernel; the table otherwise)
        pl.table = !(env_.spec && fam == FAM_HEADLINE) || env_.famrt;
        pl.keep_params = keep_params(pl.nt, pl.table, fam);
        pl.lds_ring = lds_ring(pl.nt, pl.table);
        return true;
    }
    // k_fused_compact<XR=2> as planned: the plain pass (trial = 0: x_d = x + d formed into xd, z into zarg unless null) or
    // the trial-given pass (trial = 1: the point given in xd, its z and res into zarg, resarg).  form_[C_FUSED_IT] names
    // the instantiation that the same values select (tests assert it, bench.py matches profiles on it).
    void launch_xr2(const GatePlan& pl, CompactCoef<CM> C, int trial, T* xd, T* zarg, T* resarg) {
        CompactVecs<T, CM> XV;
        XV.m = CM;
        for (int i = 0; i < CM; ++i) { XV.S[i] = pl.S[i]; XV.Y[i] = nullptr; }
        C.gam0 = pl.gam0;
        const T gam = (T)pl.gamma;
        auto go = [&](auto kernel) {
            launch(C_FUSED_IT, kernel, pl.gfc, XV, C, pl.x, (const T*)nullptr, P, gam, xd, zarg, resarg, (T*)nullptr,
                   (T*)nullptr, n, parts_.p, (int)SL_TRIAL);
        };
        if (pl.table) {
            C.uni_rt = pl.uni; C.trial_rt = trial;
            // the plain pass with uniform penalties has compile-time instantiations (fp64); run-time UNI / TRIAL otherwise
            FusedFn<T> fn = (trial == 0 && !env_.famrt) ? family_kernel<T>(pl.fam, pl.nt, pl.uni) : nullptr;
            const bool ct = fn != nullptr;
            if (!fn) fn = family_kernel<T>(pl.fam, pl.nt, -1);
            if (!fn) throw Error(BZ_ERR_STATE, "no one-pass kernel instantiation for this oracle family");
            form_[C_FUSED_IT] = std::string("k_fused_compact<XR=2,UNI=") + (ct ? std::to_string(pl.uni) : std::string("-1")) + ",NT=" +
                                std::to_string(pl.nt ? 1 : 0) + ",TRIAL=" + (ct ? "0" : "-1") + ",FAM=" + std::to_string(pl.fam) + ">";
            go(fn);
            return;
        }
        form_[C_FUSED_IT] = std::string("k_fused_compact<XR=2,UNI=") + char('0' + pl.uni) + (pl.nt ? ",NT=1" : ",NT=0") +
                            (trial ? ",TRIAL=1" : ",TRIAL=0") + (pl.keep_params ? ",PP=1" : "") + (pl.lds_ring ? ",LQ=1>" : ">");
        with_bool(trial != 0, [&](auto tr) {
            with_uni(pl.uni, [&](auto un) {
                constexpr int TR = decltype(tr)::value, UNI = decltype(un)::value;
                if (pl.lds_ring) {      // (fp64 only: lds_ring)
                    if constexpr (sizeof(T) == 8) {
                        if (pl.keep_params) go(k_fused_compact<T, CM, true, true, true, 2, UNI, TR, FAM_HEADLINE, 1, 1>);
                        else go(k_fused_compact<T, CM, true, true, true, 2, UNI, TR, FAM_HEADLINE, 0, 1>);
                    }
                } else if (pl.nt && pl.keep_params) go(k_fused_compact<T, CM, true, true, true, 2, UNI, TR, FAM_HEADLINE, 1>);
                else if (pl.nt) go(k_fused_compact<T, CM, true, true, true, 2, UNI, TR, FAM_HEADLINE, 0>);
                else go(k_fused_compact<T, CM, false, true, true, 2, UNI, TR, FAM_HEADLINE, 0>);
            });
        });
    }
    // launch the NEXT iteration's pass now, gated on the host record, planned for this one (x_d at ring position xd, m_now
    // pairs) ending the plain way: trial accepted, pair inserted, same gamma — the ring one step on, one more pair — and (not
    // known yet) no z store
    void gate_prelaunch(int xd, int m_now) {
        double gr[NXR];
        for (int i = 0; i < NXR; ++i) gr[i] = gring_[i];
        gr[xd] = (double)state_.gamma;
        GatePlan pl;
        if (!xr2_plan(xd, std::min(m_now + 1, state_.lbfgs.M), gr, xr_run_ + 1, false, pl)) return;
        gate_alloc();
        CompactCoef<CM> C2;
        std::memset(&C2, 0, sizeof(C2));
        // (BZ_GATE_SPIN: the poll bounds, for the test of the fall-back)
        C2.gate_spin_host = env_.gate_spin ? env_.gate_spin : GATE_SPIN_HOST;
        C2.gate_spin_dev = env_.gate_spin ? 8u * env_.gate_spin : GATE_SPIN_DEV;
        C2.gate_seq = ++gate_seq_; C2.gate_host = gate_host_dev_; C2.gate_dev = gate_dev_.p; C2.gate_timeout = ptimeout_dev_;
        mv(xr2_streams(pl.m_now));
        gate_bytes_ = pending_bytes_;
        launch_xr2(pl, C2, 0, pl.xd, (T*)nullptr, (T*)nullptr);
        gate_plan_ = pl; gate_pending_ = true;
    }
    void gate_release(const CompactCoef<CM>& C, T* zstore) {
        if (gate_sabotage_ > 0 && --gate_sabotage_ == 0) {      // (test) forget this release: the launch times out at its gate
            gate_pending_ = false; ++n_gated_;
            return;
        }
        // 12 values (u1, u2h, H0, the z address) as tagged half-words: any order, each word validates itself
        double vals[13] = {0};
        for (int i = 0; i < CM; ++i) { vals[i] = C.u1[i]; vals[5 + i] = C.u2h[i]; }
        vals[10] = C.H0;
        const unsigned long long zbits = (unsigned long long)(uintptr_t)zstore;
        std::memcpy(&vals[11], &zbits, sizeof(double));
        const unsigned long long tag = (unsigned long long)ll_tag(gate_seq_) << 32;
        volatile unsigned long long* w = gate_host_->w;
        for (int i = 0; i < 13; ++i) {
            unsigned long long bits;
            std::memcpy(&bits, &vals[i], sizeof(bits));
            w[2 * i] = tag | (bits & 0xFFFFFFFFull);
            w[2 * i + 1] = tag | (bits >> 32);
        }
        std::atomic_thread_fence(std::memory_order_release);
        gate_pending_ = false; ++n_gated_;
        if (zstore) bytes_all_[C_FUSED_IT] += (double)n * sizeof(T);
    }
    void gate_abort() {
        if (!gate_pending_) return;
        *(volatile unsigned long long*)&gate_host_->w[31] = ((unsigned long long)ll_tag(gate_seq_) << 32) | 1ull;
        std::atomic_thread_fence(std::memory_order_release);
        gate_pending_ = false; ++n_gate_aborts_;
        bytes_all_[C_FUSED_IT] -= gate_bytes_; launches_all_[C_FUSED_IT] -= 1;      // (it left without moving anything)
    }
    bool prof_would_pick(int cat) const {
        return ((prof_mask >> cat) & 1u) && (prof_count[cat] % prof_period) == 0;
    }

    // profiling
    struct ProfRec { int cat; hipEvent_t a, b; double bytes; };
    unsigned prof_mask = 0, prof_period = 1;
    // Bytes every launch is DESIGNED to move (its read + write streams x their length x sizeof(T)), noted by mv()
    // right before the launch: counted for every launch of a category (bytes_all_) and for the launches that
    // carry timing events (bytes_timed_), so that a sustained rate is moved bytes / measured time of the SAME
    // launches whatever mix of kernel forms ran.  form_[cat]: template form of the category's last launch.
    double pending_bytes_ = 0.0;
    const char* pending_form_ = nullptr;
    void nm(const char* kernel_name) { pending_form_ = kernel_name; }
    double bytes_all_[BZ_NUM_KERNEL_CATEGORIES] = {0}, bytes_timed_[BZ_NUM_KERNEL_CATEGORIES] = {0};
    int64_t launches_all_[BZ_NUM_KERNEL_CATEGORIES] = {0};
    std::string form_[BZ_NUM_KERNEL_CATEGORIES];
    void mv(double passes, int64_t len = -1) { pending_bytes_ += passes * (double)(len < 0 ? n : len) * sizeof(T); }
    // parameter vectors an element-wise kernel streams (load_params)
    int pstreams(bool need_f, bool need_al, bool need_g) const {
        int k = 0;
        if (need_f && P.f_kind == BZ_F_DIAG_QUADRATIC) k += 2;
        if (need_al) k += 2 - (P.uni >= 1 ? 1 : 0) - (P.uni >= 2 ? 1 : 0) + (P.D_lo_vec ? 1 : 0) + (P.D_hi_vec ? 1 : 0);
        if (need_g) k += (P.g_u && (P.g_kind == BZ_G_NORM_L1_BOX || P.g_kind == BZ_G_NORM_L0_BOX || P.g_kind == BZ_G_NORM_LP_BOX) ? 1 : 0) +
                         (P.scale_vec() ? 1 : 0) + (P.g_lo_vec ? 1 : 0) + (P.g_hi_vec ? 1 : 0);
        return k;
    }
    void account(int cat, ProfRec* r) {
        bytes_all_[cat] += pending_bytes_; launches_all_[cat] += 1;
        if (r) r->bytes = pending_bytes_;
        pending_bytes_ = 0.0;
        if (pending_form_) { form_[cat] = pending_form_; pending_form_ = nullptr; }
    }
    unsigned prof_count[BZ_NUM_KERNEL_CATEGORIES] = {0};
    bool prof_pick(int cat) {
        if (!((prof_mask >> cat) & 1u)) return false;
        return (prof_count[cat]++ % prof_period) == 0;
    }
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[BZ_NUM_KERNEL_CATEGORIES] = {0};
    int64_t prof_n[BZ_NUM_KERNEL_CATEGORIES] = {0};

    hipEvent_t get_event() {
        if (!ev_pool.empty()) { hipEvent_t e = ev_pool.back(); ev_pool.pop_back(); return e; }
        hipEvent_t e; BZ_HIP(hipEventCreate(&e)); return e;
    }
    void drain_prof() {
        if (prof_recs.empty()) return;
        BZ_HIP(hipStreamSynchronize(ctx->stream));
        for (auto& r : prof_recs) {
            float ms = 0; BZ_HIP(hipEventElapsedTime(&ms, r.a, r.b));
            prof_ms[r.cat] += ms; prof_n[r.cat] += 1; bytes_timed_[r.cat] += r.bytes;
            ev_pool.push_back(r.a); ev_pool.push_back(r.b);
        }
        prof_recs.clear();
    }

    template <class K, class... A> void launch(int cat, K kernel, int g, A... args) {
        launch_b(cat, kernel, g, BLOCK, args...);
    }
    template <class K, class... A> void launch2d(int cat, K kernel, int gx, int gy, A... args) {
        launch_b(cat, kernel, dim3(gx, gy), BLOCK, args...);
    }
    template <class K, class... A> void launch_b(int cat, K kernel, dim3 g, int block, A... args) {
        ProfRec r{cat, nullptr, nullptr, 0.0};
        const bool prof_on = prof_pick(cat);
        account(cat, prof_on ? &r : nullptr);
        if (prof_on) {
            // start/stop events bound to the dispatch itself: kernel time without the launch gap
            r.a = get_event(); r.b = get_event();
            hipExtLaunchKernelGGL(kernel, g, dim3(block), 0, ctx->stream, r.a, r.b, 0, args...);
            prof_recs.push_back(r);
            if (prof_recs.size() > 8192) drain_prof();
        } else {
            hipLaunchKernelGGL(kernel, g, dim3(block), 0, ctx->stream, args...);
        }
        BZ_HIP(hipGetLastError());
    }

    void upload(DBuf<T>& dst, const void* src, int64_t cnt) {
        dst.alloc(cnt);
        copy_in(dst.p, src, cnt);
    }
    void copy_in(T* dst, const void* src, int64_t cnt) {
        if (!src) throw Error(BZ_ERR_ARG, "null input pointer");
        BZ_HIP(hipMemcpyAsync(dst, src, cnt * sizeof(T), hipMemcpyDefault, ctx->stream));
        BZ_HIP(hipStreamSynchronize(ctx->stream));
    }
    void copy_out(void* dst, const T* src, int64_t cnt) {
        if (!dst) throw Error(BZ_ERR_ARG, "null output pointer");
        BZ_HIP(hipMemcpyAsync(dst, src, cnt * sizeof(T), hipMemcpyDefault, ctx->stream));
        BZ_HIP(hipStreamSynchronize(ctx->stream));
    }
    void require_active() const {
        if (!active) throw Error(BZ_ERR_STATE, "no solve in progress (call bz_panoc_begin first)");
    }

    // ---- row-block-sharded stencil: halo rows through IPC-mapped fine-grained buffers -------------------
    // region layout: rows[parity][side][ny] of T (side 0 = north halo, written by the previous rank; side 1 =
    // south halo, written by the next rank), then flags[parity][side] (64-byte aligned)
    void* halo_local_ = nullptr;
    void* halo_prev_ = nullptr;
    void* halo_next_ = nullptr;
    bool halo_connected_ = false;
    unsigned long long hseq_ = 0;
    size_t halo_rows_bytes() const { return ((size_t)4 * desc.f_grid_ny * sizeof(T) + 63) / 64 * 64; }
    size_t halo_bytes() const { return halo_rows_bytes() + 64; }
    static T* halo_row(void* base, int par, int side, int64_t ny) { return (T*)base + (size_t)(par * 2 + side) * ny; }
    unsigned long long* halo_flag(void* base, int par, int side) const {
        return (unsigned long long*)((char*)base + halo_rows_bytes()) + (par * 2 + side);
    }
    bool sharded_stencil() const { return desc.f_kind == BZ_F_STENCIL5 && ctx->nranks > 1; }
   public:
    void halo_export(void* handle64) override {
        if (!sharded_stencil()) throw Error(BZ_ERR_STATE, "halo buffers exist only for a sharded Stencil5pt problem");
        BZ_HIP(hipSetDevice(ctx->device));
        if (!halo_local_) {
            BZ_HIP(hipExtMallocWithFlags(&halo_local_, halo_bytes(), hipDeviceMallocFinegrained));
            BZ_HIP(hipMemset(halo_local_, 0, halo_bytes()));
            BZ_HIP(hipDeviceSynchronize());
        }
        hipIpcMemHandle_t h;
        BZ_HIP(hipIpcGetMemHandle(&h, halo_local_));
        std::memcpy(handle64, &h, sizeof(h));
    }
    // handles of the previous and the next rank's halo regions (ignored at the two ends of the rank order)
    void halo_connect(const void* prev64, const void* next64) override {
        if (!halo_local_) throw Error(BZ_ERR_STATE, "bz_problem_halo_export must be called first");
        BZ_HIP(hipSetDevice(ctx->device));
        auto open = [&](const void* h64, void** out) {
            if (!h64) throw Error(BZ_ERR_ARG, "missing neighbour halo handle");
            hipIpcMemHandle_t h;
            std::memcpy(&h, h64, sizeof(h));
            BZ_HIP(hipIpcOpenMemHandle(out, h, hipIpcMemLazyEnablePeerAccess));
        };
        if (ctx->rank > 0 && !halo_prev_) open(prev64, &halo_prev_);
        if (ctx->rank + 1 < ctx->nranks && !halo_next_) open(next64, &halo_next_);
        halo_connected_ = true;
    }
   private:
    // exchange the boundary rows of v with the neighbours; the halo the stencil kernel then reads
    StencilHalo<T> halo_exchange(const T* v) {
        if (!sharded_stencil()) return StencilHalo<T>{nullptr, nullptr};
        if (!halo_connected_) throw Error(BZ_ERR_STATE, "sharded Stencil5pt: bz_problem_halo_connect has not been called");
        const int64_t gny = desc.f_grid_ny, rows = desc.f_grid_nx;
        const unsigned long long seq = ++hseq_;
        const int par = (int)(seq & 1ull);
        HaloArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        a.first_row = v; a.last_row = v + (size_t)(rows - 1) * gny;
        a.seq = seq; a.ny = gny; a.timeout = ptimeout_dev_;
        if (halo_prev_) { a.prev_south = halo_row(halo_prev_, par, 1, gny); a.prev_flag = halo_flag(halo_prev_, par, 1); }
        if (halo_next_) { a.next_north = halo_row(halo_next_, par, 0, gny); a.next_flag = halo_flag(halo_next_, par, 0); }
        a.my_north_flag = halo_flag(halo_local_, par, 0);
        a.my_south_flag = halo_flag(halo_local_, par, 1);
        launch_b(C_GATHER, k_halo_exchange<T>, 1, XBLOCK, a);
        return StencilHalo<T>{halo_prev_ ? halo_row(halo_local_, par, 0, gny) : nullptr,
                              halo_next_ ? halo_row(halo_local_, par, 1, gny) : nullptr};
    }
    // ---- dense constraint in ONE pass over A (k_dense_fused) ------------------------------------------
    bool dense_fused_broken_ = false;
    int64_t n_dense_fallbacks_ = 0, n_dense_onepass_ = 0;
    int df_kp_ = 0, df_G_ = 0, df_groups_ = 0;
    int64_t df_rpg_ = 0;
    unsigned long long df_seq_ = 1;
    DBuf<unsigned long long> df_mail_;
    // the plan for an ny x n matrix on this device, or df_kp_ = 0 when the kernel does not apply
    template <int KP_> static int dense_occupancy() {
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)k_dense_fused<T, KP_>, FBLOCK, 0) != hipSuccess) {
            (void)hipGetLastError();
            occ = 0;
        }
        return occ;
    }
    void dense_fused_plan() {
        df_kp_ = 0;
        constexpr int N = PackN<T>::N;
        // (a dense f beside the dense c, and the slack form: the two-kernel form — no row epilogue for them in k_dense_fused)
        if (desc.c_kind != BZ_C_DENSE_AFFINE || x_replicated || slack || dense_f || (n % N) != 0) return;
        if (desc.D_kind >= BZ_D_VC_PAIRS) return;
        const int64_t npk = n / N;
        // KP packs per row and lane: kp_full fills a CU's registers with ONE workgroup's ring of tiles — the fewest slices per
        // row group, so the fewest partners per exchange (narrower slices: 16 or 32 partners, and several workgroups per CU,
        // measured 20-60 % slower on cfg 4); the narrower forms serve matrices with few columns
        const int kp_full = std::is_same<T, float>::value ? 4 : 2;
        int kp = kp_full;
        if (cenv_.dense_kp) kp = std::max(1, std::min(kp_full, *cenv_.dense_kp));
        while (kp > 1 && kp != 2 && kp != 4) --kp;
        while (kp > 1 && (int64_t)FBLOCK * (kp / 2) >= npk) kp /= 2;       // (a matrix narrower than one slice: more row groups instead)
        while (kp < kp_full && (npk + (int64_t)FBLOCK * kp - 1) / ((int64_t)FBLOCK * kp) > FG_MAX) kp *= 2;
        const int64_t G = (npk + (int64_t)FBLOCK * kp - 1) / ((int64_t)FBLOCK * kp);
        // co-resident workgroups: what the runtime says fits a CU, at most what the launch bounds ask for (the groups' workgroups
        // wait for each other: a grid beyond the resident set would only ever time out)
        int occ = 0;
        if (kp == 1) occ = dense_occupancy<1>();
        else if (kp == 2) occ = dense_occupancy<2>();
        else if constexpr (std::is_same<T, float>::value) occ = dense_occupancy<4>();
        const int64_t slots = (int64_t)num_cus * std::min(occ, kp_full / kp);
        if (G > FG_MAX || G > slots) return;
        int64_t groups = std::max<int64_t>(1, std::min<int64_t>(slots / G, (ny + FT - 1) / FT));
        int64_t rpg = (ny + groups - 1) / groups;
        rpg = (rpg + FT - 1) / FT * FT;
        groups = (ny + rpg - 1) / rpg;
        if (rpg > FRC) return;                                          // (a group's row parameters must fit the kernel's LDS cache)
        df_kp_ = kp; df_G_ = (int)G; df_groups_ = (int)groups; df_rpg_ = rpg;
        df_mail_.alloc((size_t)groups * FMS * FG_MAX * FT * 2);
    }
    bool dense_fused_on() const { return cenv_.dense_fused && df_kp_ > 0 && !dense_fused_broken_; }
    // gradient!'s dense part in one pass over A: c(point) -> CX_ (and cx_keep_), the row-group partials of A'yhat -> GT_,
    // the penalty partials -> slot_pen
    void dense_fused_launch(const T* x, int slot_pen) {
        DenseFusedArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        a.A = A_.p; a.x = x; a.b = cb_.p; a.cx = CX_.p; a.cx2 = cx_keep_; a.part = GT_.p; a.pstride = npad;
        a.ny = ny; a.n = n; a.G = df_G_; a.ngroups = df_groups_; a.rows_per_group = df_rpg_;
        a.seq0 = df_seq_; a.mail = df_mail_.p; a.timeout = ptimeout_dev_;
        a.spin = cenv_.dense_spin ? cenv_.dense_spin : FSPIN_LIMIT;
        a.parts = parts_.p; a.slot_pen = slot_pen;
        df_seq_ += (unsigned long long)(df_rpg_ / FT) + 2ull * FNB;      // (every step posts, the padding steps of the last ring turn too)
        // (test) slice 0 of every group posts under tags nobody waits for: the polls give up
        if (cenv_.test_dense_timeout > 0 && ++dense_sabotage_count_ == cenv_.test_dense_timeout) a.sabotage = 1;
        if (cenv_.test_dense_timeout == -2) a.sabotage = 2;      // (timing experiment: no exchange)
        // the matrix once; x, b and the penalty vectors over the rows; c(x) out; the row-group partials
        mv((double)ny, n); mv(1, n); mv(2 + pstreams(false, true, false) + (cx_keep_ ? 1 : 0), ny); mv(df_groups_, npad);
        const int g = df_groups_ * df_G_;
        if (df_kp_ == 1) { nm("k_dense_fused<KP=1>"); launch_b(C_GEMV, k_dense_fused<T, 1>, g, FBLOCK, a, P); }
        else if (df_kp_ == 2) { nm("k_dense_fused<KP=2>"); launch_b(C_GEMV, k_dense_fused<T, 2>, g, FBLOCK, a, P); }
        else if constexpr (std::is_same<T, float>::value) { nm("k_dense_fused<KP=4>"); launch_b(C_GEMV, k_dense_fused<T, 4>, g, FBLOCK, a, P); }
        else throw Error(BZ_ERR_STATE, "k_dense_fused: no instantiation");
        slot_n[slot_pen] = df_groups_;
        ++n_dense_onepass_;
    }
    int dense_sabotage_count_ = 0;
    // ---- row-sharded dense constraint: x replicated, A' yhat summed over the ranks --------------------
    // region layout: slots[parity][rank][npad] of T, then flags[parity][rank]
    bool x_replicated = false;
    DBuf<T> JL_;                     // this rank's partial of A' yhat
    void* ar_local_ = nullptr;
    void* ar_peer_[P2P_MAXRANKS] = {};
    bool ar_connected_ = false;
    DBuf<unsigned long long> ar_done_;
    unsigned long long ar_done_base_ = 0;
    unsigned long long arseq_ = 0;
    size_t ar_slots_bytes() const { return ((size_t)2 * ctx->nranks * npad * sizeof(T) + 63) / 64 * 64; }
    size_t ar_bytes() const { return ar_slots_bytes() + 2 * P2P_MAXRANKS * sizeof(unsigned long long); }
    T* ar_slot(void* base, int par, int r) const { return (T*)base + (size_t)(par * ctx->nranks + r) * npad; }
    unsigned long long* ar_flag(void* base, int par, int r) const {
        return (unsigned long long*)((char*)base + ar_slots_bytes()) + (par * P2P_MAXRANKS + r);
    }
   public:
    void allreduce_export(void* handle64) override {
        if (!x_replicated) throw Error(BZ_ERR_STATE, "all-reduce regions exist only for a row-sharded DenseAffine problem");
        BZ_HIP(hipSetDevice(ctx->device));
        if (!ar_local_) {
            BZ_HIP(hipExtMallocWithFlags(&ar_local_, ar_bytes(), hipDeviceMallocFinegrained));
            BZ_HIP(hipMemset(ar_local_, 0, ar_bytes()));
            BZ_HIP(hipDeviceSynchronize());
        }
        hipIpcMemHandle_t h;
        BZ_HIP(hipIpcGetMemHandle(&h, ar_local_));
        std::memcpy(handle64, &h, sizeof(h));
    }
    void allreduce_connect(const void* handles) override {
        if (!ar_local_) throw Error(BZ_ERR_STATE, "bz_problem_allreduce_export must be called first");
        if (!handles) throw Error(BZ_ERR_ARG, "null handles");
        BZ_HIP(hipSetDevice(ctx->device));
        for (int r = 0; r < ctx->nranks; ++r) {
            if (r == ctx->rank) { ar_peer_[r] = ar_local_; continue; }
            if (ar_peer_[r]) continue;
            hipIpcMemHandle_t h;
            std::memcpy(&h, (const char*)handles + (size_t)r * 64, 64);
            BZ_HIP(hipIpcOpenMemHandle(&ar_peer_[r], h, hipIpcMemLazyEnablePeerAccess));
        }
        ar_connected_ = true;
    }
   private:
    // sum JL_ over the ranks: returns the chunk array (nranks chunks of npad) k_gemv_t_finish then folds
    const T* allreduce_partials() {
        if (!ar_connected_) throw Error(BZ_ERR_STATE, "row-sharded DenseAffine: bz_problem_allreduce_connect has not been called");
        const unsigned long long seq = ++arseq_;
        const int par = (int)(seq & 1ull);
        VecXchgArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        a.local = JL_.p; a.seq = seq; a.npad = npad; a.nranks = ctx->nranks; a.timeout = ptimeout_dev_;
        for (int r = 0; r < ctx->nranks; ++r) {
            a.peer_slot[r] = ar_slot(ar_peer_[r], par, ctx->rank);
            a.peer_flag[r] = ar_flag(ar_peer_[r], par, ctx->rank);
        }
        a.my_flags = ar_flag(ar_local_, par, 0);
        const int64_t packs = npad / PackN<T>::N;
        const int g = (int)std::max<int64_t>(1, std::min<int64_t>(64, (packs + BLOCK - 1) / BLOCK));
        if (!ar_done_.p) ar_done_.alloc(16);
        ar_done_base_ += (unsigned long long)g;
        a.done = ar_done_.p; a.target = ar_done_base_;
        launch_b(C_GATHER, k_vec_allgather<T>, g, BLOCK, a);
        return ar_slot(ar_local_, par, 0);
    }

    // z of the CURRENT state into Z_[zc] if the last fused pass skipped its store:
    //   z = prox_{gamma g}(x - gamma grad L(x))   — the arithmetic of k_algrad_elem + k_fbstep, which the fused
    //   passes reproduce bit for bit (test_fused_equals_generic_bitwise)
    // (likewise the residual res = x - z into RES_[rc] when the pass did not store it)
    // need_res = false: the caller reads z only (the solution of a subproblem, alps.jl:67): a z that the last pass stored is
    // enough, whatever the state of res (the iterate-history passes never write it)
    void ensure_z(bool need_res = true) { ensure_z(need_res, state_.gamma); }
    // gam: the gamma z and res of the current state belong to (see materialize_pairs)
    void ensure_z(bool need_res, T gam) {
        if (state_.z_valid && (state_.res_valid || !need_res)) return;
        if (begin_fb_ok()) {
            mv(1 + pstreams(true, true, true) + 1 + (state_.res_valid ? 0 : 1));
            launch(C_FB, k_zres_elem<T>, grid, (const T*)X_[xc].p, P, gam, Z_[zc].p,
                   state_.res_valid ? (T*)nullptr : RES_[rc].p, n);      // the two kernels below in one pass
        } else {
            dense_redo([&] {
                algrad(X_[xc].p, D_.p, SL_AUX);              // scratch gradient: GX_/GZ_ keep their meaning
                fbstep(X_[xc].p, D_.p, gam, Z_[zc].p, state_.res_valid ? (T*)nullptr : RES_[rc].p, SL_ZS);
            });
        }
        state_.z_valid = true; state_.res_valid = true;
    }
    // multi-GPU: fold this rank's block partials of slots [first, first+cnt) and all-gather
    // ymask (row-sharded dense c only, where x-space quantities are computed in full by every rank): the
    // slots that are sums over THIS rank's constraint rows and must be added up; the others count once
    void gather(int first, int cnt, unsigned maxmask, unsigned ymask = 0u) {
        if (!ctx->multi()) return;
        const unsigned keepmask = x_replicated ? ymask : ~0u;
        if (ctx->p2p_on) {
            if (cnt > P2P_PACK) throw Error(BZ_ERR_ARG, "pack too large for the p2p mailbox");
            XchgArgs a;
            std::memset(&a, 0, sizeof(a));
            fill_xchg(a, first, cnt, maxmask);
            a.keepmask = keepmask;
            launch_b(C_GATHER, k_exchange, cnt, 64, a);
            return;
        }
        if (cnt > 32) throw Error(BZ_ERR_ARG, "pack too large");
        SlotCounts counts;
        std::memset(&counts, 0, sizeof(counts));
        for (int i = 0; i < cnt; ++i) counts.set(i, slot_n[first + i]);
        launch_b(C_GATHER, k_pack, cnt, 64, (const double*)parts_.p, counts, first, cnt, maxmask, send_.p, ctx->rank,
                 keepmask);
        BZ_NCCL(ncclAllGather(send_.p + first, recv_.p + (size_t)first * ctx->nranks, cnt, ncclDouble,
                              ctx->comm, ctx->stream));
        for (int s = first; s < first + cnt; ++s) { grp_first[s] = first; grp_cnt[s] = cnt; }
    }
    // what k_exchange and k_exchange_collect share (a zeroed `a`): the slots, and with mailboxes the peers and the next sequence number
    void fill_xchg(XchgArgs& a, int first, int cnt, unsigned maxmask) {
        a.parts = parts_.p; a.first = first; a.cnt = cnt; a.maxmask = maxmask;
        for (int i = 0; i < cnt; ++i) a.counts.set(i, slot_n[first + i]);
        a.rank = 0; a.nranks = 1;
        if (ctx->p2p_on) {
            a.rank = ctx->rank; a.nranks = ctx->nranks; a.seq = ++ctx->xseq;
            a.recv = recv_.p + (size_t)first * ctx->nranks;
            a.mbox_local = (P2PWords*)ctx->mbox_local;
            for (int r = 0; r < ctx->nranks; ++r) a.mbox_peer[r] = (P2PWords*)ctx->mbox_peer[r];
            for (int s = first; s < first + cnt; ++s) { grp_first[s] = first; grp_cnt[s] = cnt; }
        }
        a.timeout = ptimeout_dev_;
    }
    // the arguments of the fold + (p2p) exchange + read-back of slots [first, first + cnt): with mailboxes the exchange over
    // the ranks, without (one rank, no p2p context) the local fold alone
    XCollectArgs make_xcollect(int first, int cnt, unsigned maxmask) {
        if (cnt > P2P_PACK) throw Error(BZ_ERR_ARG, "pack too large for the p2p mailbox");
        XCollectArgs b;
        std::memset(&b, 0, sizeof(b));
        fill_xchg(b.x, first, cnt, maxmask);
        b.x.keepmask = ~0u;
        b.host_out = host_out_dev_;
        b.ticket = ++collect_seq;
        return b;
    }
    // p2p transport: k_exchange and the read-back in one launch; returns the ticket wait_host must see
    unsigned long long exchange_collect(int first, int cnt, unsigned maxmask) {
        XCollectArgs b = make_xcollect(first, cnt, maxmask);
        launch_b(C_GATHER, k_exchange_collect, cnt, 64, b);
        return b.ticket;
    }
    ScalarSrc src(int slot) const {
        if (!ctx->multi()) return ScalarSrc{parts_.p + (size_t)slot * PSTRIDE, slot_n[slot], 1};
        const int f = grp_first[slot], c = grp_cnt[slot];
        return ScalarSrc{recv_.p + (size_t)f * ctx->nranks + (slot - f), ctx->nranks, c};
    }
    // fold the listed slots (bit i of maxmask: i-th listed slot is a max) and read them back
    std::vector<double> collect_range(int first, int cnt, unsigned maxmask) {
        const unsigned long long ticket = collect_launch_range(first, cnt, maxmask);
        return wait_host(cnt, ticket);
    }
    std::vector<double> collect(std::initializer_list<int> slots, unsigned maxmask) {
        CollectArgs a;
        a.n = 0; a.maxmask = maxmask;
        for (int s : slots) a.src[a.n++] = src(s);
        return collect_run(a);
    }
    // launch the read-back of slots [first, first + cnt) without waiting; wait_host(cnt, ticket) later
    unsigned long long collect_launch_range(int first, int cnt, unsigned maxmask) {
        CollectArgs a;
        a.n = cnt; a.maxmask = maxmask;
        for (int i = 0; i < cnt; ++i) a.src[i] = src(first + i);
        collect_launch(a);
        return a.ticket;
    }
    std::vector<double> collect_run(CollectArgs& a) {
        collect_launch(a);
        return wait_host(a.n, a.ticket);
    }
    void collect_launch(CollectArgs& a) {
        a.ticket = ++collect_seq;
        bool unit = true;
        for (int i = 0; i < a.n; ++i) unit = unit && a.src[i].stride == 1;
        if (unit) launch_b(C_COLLECT, k_collect_w, a.n, 64, a, host_out_dev_);
        else launch(C_COLLECT, k_collect, a.n, a, host_out_dev_);
    }
    // what a kernel's bounded poll reported in *ptimeout_ (read once the stream has run): cleared, and thrown as the error
    // that names it
    [[noreturn]] void raise_timeout() {
        const int code = *ptimeout_;
        *ptimeout_ = 0;
        if (code == 1 && ctx->nranks == 1) throw PersistTimeout();
        if (code == 6 || code == 7) throw GateTimeout(code);
        if (code == 8) {      // (whoever can redo its work does; every later evaluation takes the two-kernel form)
            dense_fused_broken_ = true; ++n_dense_fallbacks_;
            throw DenseFusedTimeout();
        }
        throw Error(code == 1 ? BZ_ERR_HIP : BZ_ERR_COMM,
                    code == 1 ? "persistent two-loop kernel: grid barrier timed out (blocks not co-resident?)"
                    : code == 2 ? "p2p scalar exchange timed out waiting for a peer rank"
                    : code == 4 ? "stencil halo exchange timed out waiting for a neighbour rank"
                    : code == 5 ? "dense-constraint all-reduce timed out waiting for a peer rank"
                    : code == 6 ? "a pre-launched pass timed out at its gate (the host never released it)"
                    : code == 7 ? "a pre-launched pass: workgroups timed out waiting for workgroup 0 to open the gate"
                                : "persistent two-loop kernel: p2p phase exchange timed out waiting for a peer rank");
    }
    // An AL gradient outside an iteration — eval_al_gradient, a gradient of the state asked for, z re-materialised: `run`
    // queues it (and its read-back, if it has one).  A one-pass launch among it that timed out (reported at the read-back, or
    // here once the stream has run) is forgotten and `run` is redone: dense_fused_on() is off now, so in the two-kernel form.
    // (Inside step() the iteration's own read-back sees it and step() redoes the iteration from the state it started from.)
    template <class F> void dense_redo(F&& run) {
        const int64_t launched = n_dense_onepass_;
        try {
            run();
            if (n_dense_onepass_ != launched) {
                BZ_HIP(hipStreamSynchronize(ctx->stream));
                std::atomic_thread_fence(std::memory_order_acquire);
                if (*ptimeout_) raise_timeout();
            }
        } catch (const DenseFusedTimeout&) {
            if (ctx->nranks > 1 || gate_pending_) throw;
            BZ_HIP(hipStreamSynchronize(ctx->stream));
            *ptimeout_ = 0;
            run();
        }
    }
    // read n scalars from the pinned mailbox once both tagged words of each carry this read-back's tag
    std::vector<double> wait_host(int cnt, unsigned long long ticket) {
        struct { int n; } a{cnt};
        const unsigned long long tag = (unsigned long long)ll_tag(ticket) << 32;
        const unsigned long long himask = 0xFFFFFFFF00000000ull;
        // spin on the tickets in pinned host memory (a few microseconds after the kernel's stores land);
        // bounded: on a fault or a hang fall through to the blocking synchronisation, which reports it
        {
            volatile unsigned long long* ho = (volatile unsigned long long*)host_out_;
            const auto t_start = std::chrono::steady_clock::now();
            bool done = false;
            for (unsigned spin = 0; !done; ++spin) {
                done = true;
                for (int i = 0; i < a.n; ++i)
                    if ((ho[2 * i] & himask) != tag || (ho[2 * i + 1] & himask) != tag) { done = false; break; }
                if (!done && (spin & 0x3FFu) == 0x3FFu) {
                    if (!gate_pending_ && hipStreamQuery(ctx->stream) != hipErrorNotReady) break;     // finished or failed
                    if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(30)) break;
                }
            }
            bool complete = done;
            if (!done) {
                gate_abort();
                BZ_HIP(hipStreamSynchronize(ctx->stream));
                std::atomic_thread_fence(std::memory_order_acquire);
                // everything queued has run: the scalars are there now, or they will never be (a device poll that gave
                // up is reported below; anything else must not be read as numbers)
                complete = true;
                for (int i = 0; i < a.n; ++i)
                    if ((ho[2 * i] & himask) != tag || (ho[2 * i + 1] & himask) != tag) { complete = false; break; }
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            if (!complete && !*ptimeout_)
                throw Error(BZ_ERR_HIP, "a read-back did not arrive although the stream is idle (no kernel posted these scalars)");
        }
        if (*ptimeout_) raise_timeout();
        std::vector<double> out(a.n);
        const unsigned long long* hw = (const unsigned long long*)host_out_;
        for (int i = 0; i < a.n; ++i) {
            const unsigned long long bits = (hw[2 * i] & 0xFFFFFFFFull) | (hw[2 * i + 1] << 32);
            std::memcpy(&out[i], &bits, sizeof(double));
        }
        return out;
    }

    // forward-backward step kernel; the Newton/pow prox kinds use their own instantiation so the
    // common kinds keep their register budget
    void fbstep(const T* x, const T* g, T gam, T* z, T* res, int slot0) {
        if (generic_) { fbstep_generic(x, g, gam, z, res, slot0); return; }
        if (ragged_g) { fbstep_ragged(x, g, gam, z, res, slot0); return; }
        if (group_g) { fbstep_group(x, g, gam, z, res, slot0); return; }      // (no slack form with these kinds)
        if (slack_dense) {
            // one launch over the lifted vector, a section per half (k_fbstep_lifted)
            for (int k = 0; k < 3; ++k) slot_n[slot0 + k] = lgx_ + lgs_;
            const int vs = 1 + (g ? 1 : 0) + 1 + (res ? 1 : 0);
            mv(vs + pstreams(false, false, true), nx); mv(vs + (P.D_lo_vec ? 1 : 0) + (P.D_hi_vec ? 1 : 0), ny);
            nm(lp_g ? "k_fbstep_lifted<LP=1>" : "k_fbstep_lifted<LP=0>");
            if (lp_g) launch(C_FB, k_fbstep_lifted<T, true>, lgx_ + lgs_, x, g, gam, P, z, res, nx, ny, lgx_, lgs_, parts_.p, slot0);
            else launch(C_FB, k_fbstep_lifted<T, false>, lgx_ + lgs_, x, g, gam, P, z, res, nx, ny, lgx_, lgs_, parts_.p, slot0);
            return;
        }
        if (slack) {
            for (int k = 0; k < 3; ++k) slot_n[slot0 + k] = grid_y;
            mv(2 * (1 + (g ? 1 : 0) + 1 + (res ? 1 : 0)) + pstreams(false, false, true) + (P.D_lo_vec ? 1 : 0) + (P.D_hi_vec ? 1 : 0), nx);
            nm(lp_g ? "k_fbstep_slack<LP=1>" : "k_fbstep_slack<LP=0>");
            if (lp_g) launch(C_FB, k_fbstep_slack<T, true>, grid_y, x, g, gam, P, z, res, nx, parts_.p, slot0);
            else launch(C_FB, k_fbstep_slack<T, false>, grid_y, x, g, gam, P, z, res, nx, parts_.p, slot0);
            return;
        }
        for (int k = 0; k < 3; ++k) slot_n[slot0 + k] = grid;
        mv(1 + (g ? 1 : 0) + 1 + (res ? 1 : 0) + pstreams(false, false, true));
        nm(lp_g ? "k_fbstep<LP=1>" : "k_fbstep<LP=0>");
        if (lp_g) launch(C_FB, k_fbstep<T, true>, grid, x, g, gam, P, z, res, n, parts_.p, slot0);
        else launch(C_FB, k_fbstep<T, false>, grid, x, g, gam, P, z, res, n, parts_.p, slot0);
    }
    // g = NormL21: k_fbstep_group<KP, NT>, KP the power of two >= K.  The streams k_fbstep counts, and one entry per group of
    // a vector lambda; non-temporal loads when those streams are beyond the Infinity Cache
    void fbstep_group(const T* x, const T* g, T gam, T* z, T* res, int slot0) {
        const int64_t ngroups = n / grp_K_;
        const int gg = group_grid(ngroups, grp_KP_);
        const T* lamv = P.group_lambda_vec();
        for (int k = 0; k < 3; ++k) slot_n[slot0 + k] = gg;
        const int vs = 1 + (g ? 1 : 0) + 1 + (res ? 1 : 0);
        mv(vs); if (lamv) mv(1, ngroups);
        const bool nt = env_.nt >= 0 ? env_.nt != 0 : (double)n * sizeof(T) * vs > 340e6;
        with_bool(nt, [&](auto nt_) {
            constexpr bool NT = decltype(nt_)::value;
            auto go = [&](auto kp_) {
                constexpr int KP = decltype(kp_)::value;
                launch(C_FB, k_fbstep_group<T, KP, NT>, gg, x, g, gam, P.g_lambda, lamv, grp_K_, z, res, ngroups, parts_.p, slot0);
            };
            switch (grp_KP_) {
            case 1: nm(NT ? "k_fbstep_group<KP=1,NT=1>" : "k_fbstep_group<KP=1,NT=0>"); go(std::integral_constant<int, 1>{}); break;
            case 2: nm(NT ? "k_fbstep_group<KP=2,NT=1>" : "k_fbstep_group<KP=2,NT=0>"); go(std::integral_constant<int, 2>{}); break;
            case 4: nm(NT ? "k_fbstep_group<KP=4,NT=1>" : "k_fbstep_group<KP=4,NT=0>"); go(std::integral_constant<int, 4>{}); break;
            case 8: nm(NT ? "k_fbstep_group<KP=8,NT=1>" : "k_fbstep_group<KP=8,NT=0>"); go(std::integral_constant<int, 8>{}); break;
            case 16: nm(NT ? "k_fbstep_group<KP=16,NT=1>" : "k_fbstep_group<KP=16,NT=0>"); go(std::integral_constant<int, 16>{}); break;
            case 32: nm(NT ? "k_fbstep_group<KP=32,NT=1>" : "k_fbstep_group<KP=32,NT=0>"); go(std::integral_constant<int, 32>{}); break;
            default: nm(NT ? "k_fbstep_group<KP=64,NT=1>" : "k_fbstep_group<KP=64,NT=0>"); go(std::integral_constant<int, 64>{}); break;
            }
        });
    }
    // g = GroupLasso: k_fbstep_ragged<L, NT, L1, LONG>, L lanes per group from the mean size, LONG where a group exceeds the
    // RAGGED_HOLD trips held in registers.  The streams k_fbstep counts, the pointer (and a vector lambda) once per group, and
    // x and g a second time for the waves that sweep twice (grp_swept_)
    void fbstep_ragged(const T* x, const T* g, T gam, T* z, T* res, int slot0) {
        const int gg = group_grid(grp_ng_, grp_L_);
        const T* lamv = P.group_lambda_vec();
        const T l1 = (T)desc.g_l1;
        for (int k = 0; k < 3; ++k) slot_n[slot0 + k] = gg;
        const int vs = 1 + (g ? 1 : 0) + 1 + (res ? 1 : 0);
        mv(vs); if (lamv) mv(1, grp_ng_);
        mv((double)sizeof(int64_t) / sizeof(T), grp_ng_ + 1);
        mv(1 + (g ? 1 : 0), grp_swept_);
        const bool nt = env_.nt >= 0 ? env_.nt != 0 : (double)n * sizeof(T) * vs > 340e6;
        const bool lng = grp_max_ > (int64_t)RAGGED_HOLD * grp_L_;
        const bool l1p = desc.g_l1 > 0;
        with_bool(nt, [&](auto nt_) {
            with_bool(l1p, [&](auto l1_) {
                with_bool(lng, [&](auto lng_) {
                    // (L = 1: every group has one element, lng is false; its LONG forms are not instantiated)
                    auto go = [&](auto l_) {
                        constexpr int L = decltype(l_)::value;
                        launch(C_FB, k_fbstep_ragged<T, L, decltype(nt_)::value, decltype(l1_)::value, (decltype(lng_)::value && L > 1)>,
                               gg, x, g, gam, P.g_lambda, lamv, l1, (const int64_t*)gptr_.p, z, res, grp_ng_, parts_.p, slot0);
                    };
#define BZ_RAGGED_NM(A) (nt ? (l1p ? (lng ? A "NT=1,L1=1,LONG=1>" : A "NT=1,L1=1,LONG=0>") : (lng ? A "NT=1,L1=0,LONG=1>" : A "NT=1,L1=0,LONG=0>")) \
                               : (l1p ? (lng ? A "NT=0,L1=1,LONG=1>" : A "NT=0,L1=1,LONG=0>") : (lng ? A "NT=0,L1=0,LONG=1>" : A "NT=0,L1=0,LONG=0>")))
                    switch (grp_L_) {
                    case 1: nm(BZ_RAGGED_NM("k_fbstep_ragged<L=1,")); go(std::integral_constant<int, 1>{}); break;
                    case 2: nm(BZ_RAGGED_NM("k_fbstep_ragged<L=2,")); go(std::integral_constant<int, 2>{}); break;
                    case 4: nm(BZ_RAGGED_NM("k_fbstep_ragged<L=4,")); go(std::integral_constant<int, 4>{}); break;
                    case 8: nm(BZ_RAGGED_NM("k_fbstep_ragged<L=8,")); go(std::integral_constant<int, 8>{}); break;
                    case 16: nm(BZ_RAGGED_NM("k_fbstep_ragged<L=16,")); go(std::integral_constant<int, 16>{}); break;
                    case 32: nm(BZ_RAGGED_NM("k_fbstep_ragged<L=32,")); go(std::integral_constant<int, 32>{}); break;
                    default: nm(BZ_RAGGED_NM("k_fbstep_ragged<L=64,")); go(std::integral_constant<int, 64>{}); break;
                    }
#undef BZ_RAGGED_NM
                });
            });
        });
    }
    T al_value(double fsum, double pensum) const {   // auglagfun.jl:78,81-82
        T lx = T(0.5) * T(pensum);
        lx += f_value(fsum);
        lx -= musqy;
        return lx;
    }
    T f_value(double fsum) const { return fscale == T(1) ? T(fsum) : fscale * T(fsum); }
    T g_value(double gsum) const {
        switch (desc.g_kind) {
        case BZ_G_NORM_L1: case BZ_G_NORM_L1_NONNEG: case BZ_G_NORM_L1_BOX: case BZ_G_NORM_L0_BOX:
        case BZ_G_NORM_LP_NONNEG: case BZ_G_NORM_LP_BOX:
            if (P.lambda_vec()) return T(gsum);      // (the kernels summed lambda_i |z_i|)
            return P.g_lambda * T(gsum);
        case BZ_G_NORM_L21:
            if (P.group_lambda_vec()) return T(gsum);      // (the kernel summed lambda_j (scal nrm))
            return P.g_lambda * T(gsum);
        case BZ_G_GROUP_LASSO:
            // (a vector lambda, or l1 > 0: the kernel summed the finished terms)
            if (P.group_lambda_vec() || desc.g_l1 > 0) return T(gsum);
            return P.g_lambda * T(gsum);
        case BZ_G_ELASTIC_NET: return T(gsum);   // (the kernels summed the finished terms, weighted or not)
        case BZ_G_CALLBACK: return T(gsum);      // the callback returned g(z) itself
        default: return T(0);
        }
    }

    // ---- c = SparseAffine: A and A' as two CSR matrices in HBM, each with the launch plan fixed at creation
    struct SpCsr {
        DBuf<int64_t> ptr;                 // [nv + 1]: the row pointers, refined at the cuts of long rows
        DBuf<int32_t> col;
        DBuf<T> val;
        DBuf<int32_t> vrow, vpart;         // cut matrices only: virtual row -> row, and -> its slot in `part` (-1: a whole row)
        DBuf<int32_t> crow, cptr;          // the cut rows and where each one's segment sums start in `part`
        DBuf<double> part;
        int64_t rows = 0, cols = 0, nnz = 0, nv = 0, S = 0;
        int L = 1, ncut = 0;
        int64_t kw = 1;                    // values behind a gathered index (the multinomial f's matrices: K)
        SpMat<T> mat() const { return SpMat<T>{ptr.p, col.p, val.p, ncut ? vrow.p : nullptr, ncut ? vpart.p : nullptr, part.p, nv}; }
        // bytes of one pass without the per-row vectors: both CSR arrays, the row pointers (and the two virtual-row
        // tables of a cut matrix), one read of the gathered vector
        double bytes() const {
            return (double)nnz * (sizeof(T) + 4) + (double)(nv + 1) * 8 + (ncut ? (double)nv * 8 : 0.0) + (double)(cols * kw) * sizeof(T);
        }
    };
    SpCsr spA_, spAt_, spQ_;               // (Q: the sparse quadratic f; symmetric, so no transpose)
    DBuf<int64_t> spQ_rowptr_;             // a cut Q: the row pointers as given (k_spmv_q_algrad walks rows, not virtual rows)
    // the profile labels of the row launches by the epilogue's MODE (the K-wide mode over A_f — SPMM_SOFTMAX or a K-wide GLM
    // mode, one per problem — behind the others), filled at creation
    static constexpr int sp_label_at(int mode) { return mode >= SPMM_SOFTMAX ? SP_NMODES : mode; }
    std::string sp_label_[SP_NMODES + 1];
    template <class V> static void sp_upload(DBuf<V>& dst, const std::vector<V>& src) {
        dst.alloc(src.size());
        if (!src.empty()) BZ_HIP(hipMemcpy(dst.p, src.data(), src.size() * sizeof(V), hipMemcpyHostToDevice));
    }
    // Segment length: rows longer than a quarter of one wave's share of the entries are cut (the machine taken as the
    // largest grid the row kernels use, PSTRIDE workgroups of WAVES waves), never below 512 entries, a multiple of 64.
    // A function of the matrix alone.
    static int64_t sp_segment_length(int64_t nnz) {
        const int64_t share = nnz / ((int64_t)PSTRIDE * WAVES);
        return std::max<int64_t>(512, ((share / 4 + 63) / 64) * 64);
    }
    // lanes per row from the mean (virtual) row length: about four entries per lane and batch
    static int sp_lanes(int64_t nnz, int64_t nv) {
        const double mean = nv > 0 ? (double)nnz / (double)nv : 0.0;
        int L = 1;
        while (L < 64 && mean > 4.0 * L) L *= 2;
        return L;
    }
    void sp_build(SpCsr& m, int64_t rows, int64_t cols, const std::vector<int64_t>& rp, const std::vector<int32_t>& col,
                  const std::vector<T>& val) {
        m.rows = rows; m.cols = cols; m.nnz = rp[rows];
        m.S = sp_segment_length(m.nnz);
        int64_t nv = 0, nparts = 0;
        int ncut = 0;
        for (int64_t r = 0; r < rows; ++r) {
            const int64_t len = rp[r + 1] - rp[r];
            const int64_t segs = len > m.S ? (len + m.S - 1) / m.S : 1;
            nv += segs;
            if (segs > 1) { ++ncut; nparts += segs; }
        }
        if (nv > (int64_t)std::numeric_limits<int32_t>::max()) throw Error(BZ_ERR_ARG, "sparse matrix: too many row segments");
        m.nv = nv; m.ncut = ncut;
        if (ncut) {
            std::vector<int64_t> vp; std::vector<int32_t> vrow, vpart, crow, cptr;
            vp.reserve(nv + 1); vrow.reserve(nv); vpart.reserve(nv);
            int32_t np = 0;
            for (int64_t r = 0; r < rows; ++r) {
                const int64_t len = rp[r + 1] - rp[r];
                if (len > m.S) {
                    crow.push_back((int32_t)r); cptr.push_back(np);
                    for (int64_t s0 = rp[r]; s0 < rp[r + 1]; s0 += m.S) { vp.push_back(s0); vrow.push_back((int32_t)r); vpart.push_back(np++); }
                } else {
                    vp.push_back(rp[r]); vrow.push_back((int32_t)r); vpart.push_back(-1);
                }
            }
            vp.push_back(rp[rows]); cptr.push_back(np);
            sp_upload(m.ptr, vp); sp_upload(m.vrow, vrow); sp_upload(m.vpart, vpart);
            sp_upload(m.crow, crow); sp_upload(m.cptr, cptr);
            m.part.alloc((size_t)nparts);
        } else {
            sp_upload(m.ptr, rp);
        }
        sp_upload(m.col, col); sp_upload(m.val, val);
        m.L = sp_lanes(m.nnz, nv);
        if (cenv_.spmv_l) {
            const int l = *cenv_.spmv_l;
            if (l < 1 || l > 64 || (l & (l - 1))) throw Error(BZ_ERR_ARG, "BZ_SPMV_L must be a power of two in 1..64");
            m.L = l;
        }
    }
    // a host copy of the caller's CSR (rows x n), validated; `what` is the kind and `rows_name` its row count in the messages
    void sp_read(const std::string& what, const char* rows_name, int64_t rows, const int64_t* rowptr, const int32_t* colp,
                 const void* valp, int64_t nnz, std::vector<int64_t>& rp, std::vector<int32_t>& col, std::vector<T>& val,
                 int64_t ncols = -1) {
        // (ncols: the matrix's columns where they are not the problem's n — the multinomial f's A_f has n / K)
        rp.resize((size_t)rows + 1); col.resize((size_t)nnz); val.resize((size_t)nnz);
        BZ_HIP(hipMemcpy(rp.data(), rowptr, rp.size() * sizeof(int64_t), hipMemcpyDefault));
        if (nnz) {
            BZ_HIP(hipMemcpy(col.data(), colp, col.size() * sizeof(int32_t), hipMemcpyDefault));
            BZ_HIP(hipMemcpy(val.data(), valp, val.size() * sizeof(T), hipMemcpyDefault));
        }
        if (rp[0] != 0) throw Error(BZ_ERR_ARG, what + ": rowptr[0] must be 0 (row 0)");
        for (int64_t r = 0; r < rows; ++r)
            if (rp[r + 1] < rp[r] || rp[r + 1] > nnz)
                throw Error(BZ_ERR_ARG, what + ": rowptr must be non-decreasing and end at nnz (row " + std::to_string(r) + ")");
        if (rp[rows] != nnz)
            throw Error(BZ_ERR_ARG, what + ": rowptr[" + rows_name + "] must equal nnz (row " + std::to_string(rows - 1) + ")");
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t k = rp[r]; k < rp[r + 1]; ++k)
                if (col[k] < 0 || (int64_t)col[k] >= (ncols >= 0 ? ncols : n))
                    throw Error(BZ_ERR_ARG, what + (ncols >= 0 ? ": column index outside [0, n / K) (row " : ": column index outside [0, n) (row ") + std::to_string(r) + ")");
    }
    // (`lead`: what a kind puts in front — the GLM f "LOSS=…,W=…,", the multinomial f "K=…,")
    static std::string sp_form(const char* kernel, const SpCsr& m, const std::string& lead = "") {
        return std::string(kernel) + "<" + lead + "L=" + std::to_string(m.L) + ",SEG=" + (m.ncut ? "1" : "0") + ">";
    }
    void sp_name(int mode, const SpCsr& m) { sp_label_[mode] = sp_form(sp_kernel_name(mode), m); }
    // f = SparseQuadratic: Q validated on a host copy and put in HBM as one CSR matrix with A's segment and lane rules
    void sparse_f_create(const bz_problem_desc& d) {
        std::vector<int64_t> rp; std::vector<int32_t> col; std::vector<T> val;
        sp_read("SparseQuadratic", "n", nx, d.f_sp_rowptr, d.f_sp_col, d.f_sp_val, d.f_sp_nnz, rp, col, val);
        sp_build(spQ_, nx, nx, rp, col, val);
        if (spQ_.ncut) sp_upload(spQ_rowptr_, rp);        // (a cut matrix keeps the virtual rows in ptr: the rows as given too)
        sp_name(SP_Q_ALGRAD, spQ_);
        sp_name(SP_Q, spQ_);
    }
    // the refusals and argument errors the row-wise sparse kinds share, worded from the kind's row of SPARSE_ROW_F.  (The
    // multinomial f's class count is checked where its own block had it.)
    void sparse_rowwise_check(const bz_problem_desc& d) const {
        const std::string kind = spf_.name, f = std::string("sparse ") + spf_.noun + " f";
        if (slack) throw Error(BZ_ERR_UNSUPPORTED, kind + ": the slack (ALS) form is not lowered with a " + f);
        if (d.c_kind == BZ_C_DENSE_AFFINE)
            throw Error(BZ_ERR_UNSUPPORTED, kind + ": a " + f + " beside a dense c (DenseAffine) is not lowered");
        if (ctx->nranks > 1) throw Error(BZ_ERR_UNSUPPORTED, kind + ": the " + f + " is not sharded (one rank)");
        if (d.g_kind == BZ_G_CALLBACK || d.c_kind == BZ_C_CALLBACK || d.D_kind == BZ_D_CALLBACK)
            throw Error(BZ_ERR_UNSUPPORTED, kind + ": the " + f + " does not mix with host callbacks");
        if (d.f_kind == BZ_F_SPARSE_MULTINOMIAL || d.f_kind == BZ_F_SPARSE_MULTI_GLM) {
            if (d.f_classes < 2 || d.f_classes > 64)
                throw Error(BZ_ERR_ARG, kind + ": f_classes = K must be in 2 .. 64");
            if (n % d.f_classes != 0)
                throw Error(BZ_ERR_ARG, kind + ": n must be a multiple of f_classes (x is n / K rows of K)");
        }
        if (d.f_rows <= 0 || !d.f_b || !d.f_sp_rowptr || d.f_sp_nnz < 0 || (d.f_sp_nnz > 0 && (!d.f_sp_col || !d.f_sp_val)))
            throw Error(BZ_ERR_ARG, kind + " needs f_rows = m > 0, rowptr[m + 1], col[nnz], val[nnz] and " + spf_.b);
        // (32-bit: the column indices of A_f and of A_f', below m; an index into the multinomial f's X or R is formed in 64 bits)
        if (n > (int64_t)std::numeric_limits<int32_t>::max() || d.f_rows > (int64_t)std::numeric_limits<int32_t>::max())
            throw Error(BZ_ERR_ARG, kind + ": n and m must fit 32-bit indices");
    }
    // a row-wise sparse f: A_f validated on a host copy; A_f and A_f' in HBM with the segment and lane rules of A and A'
    void sparse_ls_create(const bz_problem_desc& d) {
        std::vector<int64_t> rp, tp; std::vector<int32_t> col, tcol; std::vector<T> val, tval;
        // (the K-wide kinds: A_f is m x n_f, n_f = n / K, and the transpose is built over n_f columns)
        const int64_t nf = sparse_kw ? nx / mn_K_ : nx;
        sp_read(spf_.name, "m", frows, d.f_sp_rowptr, d.f_sp_col, d.f_sp_val, d.f_sp_nnz, rp, col, val, sparse_kw ? nf : -1);
        csr_transpose(frows, nf, rp, col, val, tp, tcol, tval);
        sp_build(spF_, frows, nf, rp, col, val);
        sp_build(spFt_, nf, frows, tp, tcol, tval);
        std::string lead, lead_t;              // what the kind puts in front of L and SEG in its labels
        static const char* const loss_names[] = {"least_squares", "logistic", "huber", "squared_hinge", "poisson"};
        if (sparse_kw) {
            for (SpCsr* m : {&spF_, &spFt_}) {
                m->kw = mn_K_;
                m->L = spmm_lanes(m->nnz, m->nv, mn_KP_);
                if (cenv_.spmv_l) m->L = std::min(*cenv_.spmv_l, 64 / mn_KP_);
                if (m->ncut) m->part.alloc(m->part.n * (size_t)mn_K_);      // (a segment of a cut row leaves K sums)
            }
            lead = lead_t = "K=" + std::to_string(mn_K_) + ",";
            if (spmm_glm_mode(spf_.mode))
                lead = std::string("LOSS=") + loss_names[spf_.mode - SPMM_GLM_MODE0] + ",W=" + (desc.f_w ? "1" : "0") + "," + lead;
        } else if (spf_.mode >= SP_GLM_MODE0) {
            lead = std::string("LOSS=") + loss_names[spf_.mode - SP_GLM_MODE0] + ",W=" + (desc.f_w ? "1" : "0") + ",";
        }
        auto kernel = [&](int mode) { return sparse_kw ? spmm_kernel_name(mode) : sp_kernel_name(mode); };
        sp_label_[sp_label_at(spf_.mode)] = sp_form(kernel(spf_.mode), spF_, lead);
        for (int mode : {SP_LS_T_ALGRAD, SP_T}) sp_label_[mode] = sp_form(kernel(mode), spFt_, lead_t);
    }
    // the GLM f: w^_i = T(scale * w_i), the product in double and rounded once; without a weight vector the one number T(scale).
    // Every w_i finite and >= 0, checked on a host copy.
    void glm_weights_create(const bz_problem_desc& d) {
        const std::string what = spf_.name;     // (the multinomial f: the same two fields, the same rules)
        glm_w_uniform_ = (T)d.f_scale;
        glm_delta_ = (T)d.f_loss_delta;
        // (what the kernel multiplies by is the ROUNDED number: an fp32 problem can overflow where the double was finite)
        if (!std::isfinite((double)glm_w_uniform_))
            throw Error(BZ_ERR_ARG, what + ": f_scale must be finite and > 0 in the problem's type");
        if ((d.f_kind == BZ_F_SPARSE_GLM || d.f_kind == BZ_F_SPARSE_MULTI_GLM) && d.f_loss == BZ_LOSS_HUBER &&
            !(std::isfinite((double)glm_delta_) && glm_delta_ > T(0)))
            throw Error(BZ_ERR_ARG, what + ": the Huber loss needs f_loss_delta finite and > 0 in the problem's type");
        if (!d.f_w) return;
        std::vector<T> w((size_t)frows);
        BZ_HIP(hipMemcpy(w.data(), d.f_w, w.size() * sizeof(T), hipMemcpyDefault));
        for (int64_t r = 0; r < frows; ++r) {
            if (!(std::isfinite((double)w[r]) && w[r] >= T(0)))
                throw Error(BZ_ERR_ARG, what + ": the weights must be finite and >= 0 (row " + std::to_string(r) + ")");
            w[r] = (T)(d.f_scale * (double)w[r]);
            if (!std::isfinite((double)w[r]))
                throw Error(BZ_ERR_ARG, what + ": the weights times f_scale must be finite in the problem's type (row " + std::to_string(r) + ")");
        }
        sp_upload(glm_w_, w);
    }
    // the multinomial f: every label finite, integral and in [0, K), checked on a host copy (a bad label would silently change
    // the loss: no class lane would own the row)
    void mn_labels_check(const bz_problem_desc& d) {
        std::vector<T> b((size_t)frows);
        BZ_HIP(hipMemcpy(b.data(), d.f_b, b.size() * sizeof(T), hipMemcpyDefault));
        for (int64_t r = 0; r < frows; ++r) {
            const double v = (double)b[r];
            if (!(std::isfinite(v) && v == std::floor(v) && v >= 0 && v < (double)mn_K_))
                throw Error(BZ_ERR_ARG, "SparseMultinomial: the labels must be integers in [0, K) (row " + std::to_string(r) + ")");
        }
    }
    // lanes per class and row from the mean (virtual) row length, sp_lanes' rule under KP * L <= 64
    static int spmm_lanes(int64_t nnz, int64_t nv, int KP) {
        const double mean = nv > 0 ? (double)nnz / (double)nv : 0.0;
        int L = 1;
        while (KP * L * 2 <= 64 && mean > 4.0 * L) L *= 2;
        return L;
    }
    // go(KP, L, NT) with the run-time class width, lane count and stream policy as compile-time constants (KP * L <= 64)
    template <int KP, class F> static void spmm_with_l(int L, bool nt, F&& go) {
        with_bool(nt, [&](auto nt_) {
            constexpr int LMAX = 64 / KP;
            auto at = [&](auto l_) { go(std::integral_constant<int, KP>{}, l_, nt_); };
            if (L >= 32 && LMAX >= 32) at(std::integral_constant<int, LMAX >= 32 ? 32 : 1>{});
            else if (L >= 16 && LMAX >= 16) at(std::integral_constant<int, LMAX >= 16 ? 16 : 1>{});
            else if (L >= 8 && LMAX >= 8) at(std::integral_constant<int, LMAX >= 8 ? 8 : 1>{});
            else if (L >= 4 && LMAX >= 4) at(std::integral_constant<int, LMAX >= 4 ? 4 : 1>{});
            else if (L >= 2 && LMAX >= 2) at(std::integral_constant<int, LMAX >= 2 ? 2 : 1>{});
            else at(std::integral_constant<int, 1>{});
        });
    }
    template <class F> void spmm_with_lanes(int L, bool nt, F&& go) const {
        switch (mn_KP_) {
        case 2: spmm_with_l<2>(L, nt, go); break;
        case 4: spmm_with_l<4>(L, nt, go); break;
        case 8: spmm_with_l<8>(L, nt, go); break;
        case 16: spmm_with_l<16>(L, nt, go); break;
        case 32: spmm_with_l<32>(L, nt, go); break;
        default: spmm_with_l<64>(L, nt, go); break;
        }
    }
    // What every pass over a CSR matrix fixes before it launches: the bytes of its model — the matrix once (m.bytes(): the
    // entries, the row pointers, one read of the gathered vector) and the per-row vectors in vec_bytes —, the stream policy and
    // the grid of the fold of a cut matrix's cut rows.
    struct SpPlan { double bytes; bool nt; int gfold; };
    bool sp_nontemporal(double bytes) const { return env_.nt >= 0 ? env_.nt != 0 : bytes > 340e6; }
    SpPlan sp_plan(const SpCsr& m, double vec_bytes) const {
        const double bytes = m.bytes() + vec_bytes;
        return {bytes, sp_nontemporal(bytes), m.ncut ? (int)std::min<int64_t>(512, (m.ncut + WAVES - 1) / WAVES) : 0};
    }
    // right before the row launch: notes its bytes and its label, and returns its grid for rpb rows per workgroup (in front of
    // the fold's workgroups)
    int sp_row_grid(const SpCsr& m, const SpPlan& pl, int64_t rpb, int mode) {
        pending_bytes_ += pl.bytes;
        nm(sp_label_[sp_label_at(mode)].c_str());
        return (int)std::max<int64_t>(1, std::min<int64_t>(PSTRIDE - pl.gfold, (m.nv + rpb - 1) / rpb));
    }
    // the fold behind the row launch: `tail` is what the fold kernel takes behind the cut rows
    template <class K, class... A> void sp_fold(K kernel, SpCsr& m, const SpPlan& pl, A... tail) {
        if (!pl.gfold) return;
        pending_bytes_ += (double)m.part.n * 8 + (double)m.ncut * 8;
        launch(C_MISC, kernel, pl.gfold, (const double*)m.part.p, (const int32_t*)m.crow.p, (const int32_t*)m.cptr.p, m.ncut, tail...);
    }
    // one pass of the K-wide row kernel (spmm_kernel: SPMM_SOFTMAX or a K-wide GLM mode over A_f, SP_LS_T_ALGRAD and SP_T over A_f') and, for a cut
    // matrix, the fold of its cut rows; returns the number of block partials left in `slot`.  vec_bytes: the K-wide per-row vectors.
    template <int MODE> int spmm_pass(SpCsr& m, const T* gathered, const SpEpi<T>& E, int slot, double vec_bytes) {
        const SpPlan pl = sp_plan(m, vec_bytes);
        const int K = mn_K_;
        int g = 1;
        spmm_with_lanes(m.L, pl.nt, [&](auto kp_, auto l_, auto nt_) {
            constexpr int KP = decltype(kp_)::value, L = decltype(l_)::value;
            g = sp_row_grid(m, pl, BLOCK / (KP * L), MODE);
            launch(C_GEMV, spmm_kernel<T, KP, L, decltype(nt_)::value, MODE>(), g, m.mat(), gathered, K, E, parts_.p, slot);
            sp_fold(k_spmm_fold<T, KP, MODE>, m, pl, K, E, parts_.p, slot, g);
        });
        return g + pl.gfold;
    }
    // c = SparseAffine: validate the caller's CSR on a host copy, build A' (csr_transpose: a column's entries stay in ascending row
    // order) and put both in HBM
    void sparse_create(const bz_problem_desc& d) {
        const int64_t nnz = d.c_sp_nnz;
        std::vector<int64_t> rp, tp; std::vector<int32_t> col, tcol; std::vector<T> val, tval;
        sp_read("SparseAffine", "ny", ny, d.c_sp_rowptr, d.c_sp_col, d.c_sp_val, nnz, rp, col, val);
        csr_transpose(ny, n, rp, col, val, tp, tcol, tval);
        sp_build(spA_, ny, n, rp, col, val);
        sp_build(spAt_, n, ny, tp, tcol, tval);
        sp_name(SP_YUPD, spA_);
        sp_name(SP_T_FINISH, spAt_);
    }
    // go(L, NT) with the run-time lane count and stream policy as compile-time constants
    template <class F> static void sp_with_lanes(int L, bool nt, F&& go) {
        with_bool(nt, [&](auto nt_) {
            switch (L) {
            case 1: go(std::integral_constant<int, 1>{}, nt_); break;
            case 2: go(std::integral_constant<int, 2>{}, nt_); break;
            case 4: go(std::integral_constant<int, 4>{}, nt_); break;
            case 8: go(std::integral_constant<int, 8>{}, nt_); break;
            case 16: go(std::integral_constant<int, 16>{}, nt_); break;
            case 32: go(std::integral_constant<int, 32>{}, nt_); break;
            default: go(std::integral_constant<int, 64>{}, nt_); break;
            }
        });
    }
    // one pass of the row kernel (sp_kernel: MODE -> entry point) and, for a cut matrix, the fold of its cut rows; returns the
    // number of block partials left in `slot`
    template <int MODE> int sp_pass(SpCsr& m, const T* gathered, const SpEpi<T>& E, int slot, double vec_bytes) {
        const SpPlan pl = sp_plan(m, vec_bytes);
        int g = 1;
        sp_with_lanes(m.L, pl.nt, [&](auto l_, auto nt_) {
            constexpr int L = decltype(l_)::value;
            g = sp_row_grid(m, pl, BLOCK / L, MODE);
            launch(C_GEMV, sp_kernel<T, L, decltype(nt_)::value, MODE>(), g, m.mat(), gathered, E, parts_.p, slot);
        });
        sp_fold(k_spmv_fold<T, MODE>, m, pl, E, parts_.p, slot, g);
        return g + pl.gfold;
    }
    // rows of A: c(x) -> cx (where the caller keeps it), yhat -> yupd and the penalty partials -> slot (yupd null: c(x) alone)
    int spmv_yupd(const T* x, T* cx, T* yupd, int slot) {
        SpEpi<T> E{cb_.p, cx, yupd, nullptr, P};
        const double vecs = (1 + (cx ? 1 : 0) + (yupd ? 1 + pstreams(false, true, false) : 0)) * (double)ny * sizeof(T);
        return sp_pass<SP_YUPD>(spA_, x, E, slot, vecs);
    }
    // rows of A': grad = grad f(x) + A'yhat and the f partials -> slot
    // (the sparse quadratic f: its terms from FR_ = Q x, which spq_product has left there ; the sparse least squares or
    // logistic f: its gradient from DFX_ = A_f' r, which spls_product has left there, and no f term)
    int spmv_t_finish(const T* x, T* grad, int slot) {
        SpEpi<T> E{nullptr, nullptr, grad, x, P, sparse_f ? (const T*)FR_.p : sparse_ls ? (const T*)DFX_.p : (const T*)nullptr};
        const double vecs = ((grad ? 1 : 0) + (P.f_kind == BZ_F_DIAG_QUADRATIC || sparse_f ? 3 : 0) + (sparse_ls ? 1 : 0)) * (double)n * sizeof(T);
        return sp_pass<SP_T_FINISH>(spAt_, YU_.p, E, slot, vecs);
    }
    // rows of Q, c = Identity: the whole AL gradient — grad = (Q x + q) + yhat, the f partials -> slot, the penalty
    // partials -> slot + 1.  Per row: x, q, mu and mu*y (and D's vector bounds), the gradient.
    // One launch on k_algrad_elem's grid, whose summation tree it keeps: the scalars too are bit for bit the two-launch
    // form's.  (Accounted with the pass model of the matrix, as k_spmv_q; a cut Q reads the rows as given and its segment
    // sums in place of the virtual-row tables.)
    int spq_algrad(const T* x, T* grad, int slot) {
        SpCsr& m = spQ_;
        SpEpi<T> E{nullptr, nullptr, grad, x, P, nullptr};
        const double bytes = m.bytes() + (2 + (grad ? 1 : 0) + pstreams(false, true, false)) * (double)n * sizeof(T);
        const bool nt = sp_nontemporal(bytes);
        const SpRows R{m.ncut ? spQ_rowptr_.p : m.ptr.p, m.crow.p, m.cptr.p, m.ncut, m.S, n};
        sp_with_lanes(m.L, nt, [&](auto l_, auto nt_) {
            pending_bytes_ += bytes;
            nm(sp_label_[SP_Q_ALGRAD].c_str());
            launch(C_GEMV, k_spmv_q_algrad<T, decltype(l_)::value, decltype(nt_)::value>, grid, m.mat(), R, x, E, parts_.p, slot);
        });
        return grid;
    }
    // rows of Q: Q x -> out (null: not kept) and, with_f, the f partials -> slot (otherwise zeros)
    int spq_product(const T* x, T* out, bool with_f, int slot) {
        SpEpi<T> E{nullptr, nullptr, out, with_f ? x : (const T*)nullptr, P, nullptr};
        const double vecs = ((out ? 1 : 0) + (with_f ? 2 : 0)) * (double)n * sizeof(T);
        return sp_pass<SP_Q>(spQ_, x, E, slot, vecs);
    }
    // (pairwise D: the projection of element i needs its partner, which a row's first lane does not have)
    bool spq_fused_on() const { return cenv_.spq_fused && !(desc.D_kind >= BZ_D_VC_PAIRS && desc.D_kind <= BZ_D_XOR_PAIRS); }

    // ---- a row-wise sparse f (SparseRowF)
    // rows of A_f: r_i = w_i l'(b_i, a_i'x) -> r_out (null: not kept) and the partials of the rows' losses -> slot, in the kind's
    // mode (least squares: r = A_f x - b and sum r^2 ; the multinomial f: R = w (softmax(A_f X) - onehot(b)), m rows of K).
    // Per row: b (the multi-response GLM f: K values) and r if kept (the K-wide kinds: K values); a weight vector is one more
    // stream.
    int spls_residual(const T* x, T* r_out, int slot) {
        SpEpi<T> E{fb_.p, nullptr, r_out, nullptr, P, nullptr};
        if (spf_.weighted) { E.w = glm_w_.p; E.w_uniform = glm_w_uniform_; E.delta = glm_delta_; }
        const int kb = spmm_glm_mode(spf_.mode) ? mn_K_ : 1, kr = sparse_kw ? mn_K_ : 1;
        const double vecs = (kb + (r_out ? kr : 0) + (E.w ? 1 : 0)) * (double)frows * sizeof(T);
        int nparts = 0;
        with_sparse_f_mode(spf_.mode, [&](auto mode_) {
            constexpr int MODE = decltype(mode_)::value;
            if constexpr (MODE >= SPMM_SOFTMAX) nparts = spmm_pass<MODE>(spF_, x, E, slot, vecs);
            else nparts = sp_pass<MODE>(spF_, x, E, slot, vecs);
        });
        return nparts;
    }
    // rows of A_f', c = Identity: grad = A_f' r + yhat (r in FR_) and the penalty partials -> slot.  Per row: x, mu and mu*y
    // (and D's vector bounds), the gradient.
    int spls_t_algrad(const T* x, T* grad, int slot) {
        SpEpi<T> E{nullptr, nullptr, grad, x, P, nullptr};
        const double vecs = (1 + (grad ? 1 : 0) + pstreams(false, true, false)) * (double)n * sizeof(T);
        return sparse_kw ? spmm_pass<SP_LS_T_ALGRAD>(spFt_, FR_.p, E, slot, vecs) : sp_pass<SP_LS_T_ALGRAD>(spFt_, FR_.p, E, slot, vecs);
    }
    // rows of A_f': A_f' r -> DFX_ (r in FR_)
    void spls_product() {
        SpEpi<T> E{nullptr, nullptr, DFX_.p, nullptr, P, nullptr};
        if (sparse_kw) spmm_pass<SP_T>(spFt_, FR_.p, E, (int)SL_SCRATCH, (double)n * sizeof(T));
        else sp_pass<SP_T>(spFt_, FR_.p, E, (int)SL_SCRATCH, (double)n * sizeof(T));
    }
    // (pairwise D: the projection of element j needs its partner, which a row's first lane does not have)
    bool spls_fused_on() const { return cenv_.spls_fused && !(desc.D_kind >= BZ_D_VC_PAIRS && desc.D_kind <= BZ_D_XOR_PAIRS); }
    void spls_algrad(const T* x, T* grad, int slot0) {
        slot_n[slot0] = spls_residual(x, FR_.p, slot0);
        if (desc.c_kind == BZ_C_SPARSE_AFFINE) {
            // four launches: rows of A_f, rows of A_f' (grad f -> DFX_), rows of A, rows of A' (which adds DFX_ in)
            spls_product();
            slot_n[slot0 + 1] = spmv_yupd(x, cx_keep_, YU_.p, slot0 + 1);
            spmv_t_finish(x, grad, (int)SL_SCRATCH);                  // (no f term here: slot0 is the first launch's)
            gather(slot0, 2, 0u, 2u);
            return;
        }
        if (spls_fused_on()) {
            // c = Identity: two row launches, no element-wise kernel
            slot_n[slot0 + 1] = spls_t_algrad(x, grad, slot0 + 1);
        } else {
            // the three-launch form: the plain product, then the element-wise kernel in its mode 1
            spls_product();
            slot_n[slot0 + 1] = grid;
            mv(3 + pstreams(false, true, false));
            launch(C_ALGRAD, k_algrad_elem<T>, grid, x, P, grad, n, parts_.p, slot0, 1, (const T*)DFX_.p);
        }
        gather(slot0, 2, 0u);
    }

    // gradient!(dlx, al, x) on the device; partials -> slot0 (f terms), slot0+1 (t^2/mu)
    // row chunks of the transposed product: enough blocks to fill the chip, fixed summation order
    void plan_chunks(int64_t rows, int64_t cols, int& rpc, int& nch) const {
        const int64_t colblocks = std::max<int64_t>(1, (cols / PackN<T>::N + BLOCK - 1) / BLOCK);
        const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(rows, (2048 + colblocks - 1) / colblocks));
        rpc = (int)((rows + chunks - 1) / chunks);
        nch = (int)((rows + rpc - 1) / rpc);
    }
    // out = M p - b (b may be null): M[rows][cols] row-major
    void gemv_rows(const T* M, int64_t rows, int64_t cols, const T* p, const T* b, T* out) {
        mv((double)rows, cols); mv(b ? 2 : 1, rows); mv(1, cols);      // the matrix once, x, b and the result
        nm("k_gemv_n");
        launch(C_GEMV, k_gemv_n<T>, (int)std::min<int64_t>(rows, 65535), M, p, b, out, rows, cols);
    }
    // partials of M' v over row chunks (M[rows][cols]) into part[nch][pstride].  fp32 with cols % 64 == 0 runs on the
    // matrix cores (v_mfma_f32_16x16x4_f32), everything else on the vector ALUs; both are bound by the bytes of M.
    void gemv_cols(const T* M, int64_t rows, int64_t cols, const T* v, int rpc, int nch, T* part, int64_t pstride) {
        if constexpr (std::is_same<T, float>::value) {
            if (cols % 64 == 0 && !env_.gemv_valu) {
                mv((double)rows, cols); mv(1, rows); mv(nch, pstride);      // the matrix once, v, the row-chunk partials
                nm("k_gemv_t_mfma");
                launch2d(C_GEMV_MFMA, k_gemv_t_mfma, (int)((cols / 64 + WAVES - 1) / WAVES), nch, (const float*)M,
                         (const float*)v, (float*)part, rows, cols, rpc, pstride);
                return;
            }
        }
        const bool aligned = (cols % PackN<T>::N) == 0;
        const int colblocks = (int)(((aligned ? cols / PackN<T>::N : cols) + BLOCK - 1) / BLOCK);
        mv((double)rows, cols); mv(1, rows); mv(nch, pstride); nm("k_gemv_t");
        launch2d(C_GEMV, k_gemv_t<T>, colblocks, nch, M, v, part, rows, cols, rpc, pstride);
    }
    // eval!(cx, c, x) for the dense constraint
    void eval_c(const T* x) {
        if (desc.c_kind == BZ_C_SPARSE_AFFINE) { spmv_yupd(x, CX_.p, nullptr, (int)SL_SCRATCH); return; }
        gemv_rows(A_.p, ny, nx, x, cb_.p, CX_.p);
    }
    // dense f: leaves what k_algrad_elem / k_fvalue_elem need in FR_ / DFX_ and the f partials in slot0
    //   LeastSquares: r = A x - b ; slot0 <- <r,r> ; DFX = A' r        (ProximalOperators: 0.5||Ax-b||^2)
    //   Quadratic:    FR = Q x (value and gradient finished element-wise)
    void dense_f_eval(const T* x, int slot0, bool need_grad) {
        // (x: a vector of nx elements — the x half of the lifted vector in the slack form)
        if (desc.f_kind == BZ_F_LEAST_SQUARES) {
            gemv_rows(FA_.p, frows, nx, x, fb_.p, FR_.p);
            const int gm = (int)std::min<int64_t>(grid, std::max<int64_t>(1, (frows / PackN<T>::N + BLOCK) / BLOCK));
            mv(1, frows);
            launch(C_MISC, k_dot<T>, gm, (const T*)FR_.p, (const T*)FR_.p, T(1), frows, parts_.p, slot0);
            slot_n[slot0] = gm;
            if (need_grad) {
                gemv_cols(FA_.p, frows, nx, FR_.p, f_rows_per_chunk, f_nrowchunks, FGT_.p, npadx);
                ElemParams<T> Pz = P;
                Pz.f_kind = BZ_F_ZERO;
                mv(f_nrowchunks + 2, nx);
                launch(C_MISC, k_gemv_t_finish<T>, grid_x, (const T*)FGT_.p, f_nrowchunks, npadx, x, Pz, DFX_.p, nx,
                       parts_.p, (int)SL_SCRATCH);
            }
        } else {
            gemv_rows(FA_.p, nx, nx, x, (const T*)nullptr, FR_.p);
        }
    }
    void algrad(const T* x, T* grad, int slot0) {
        if (generic_) { algrad_generic(x, grad, slot0); return; }
        if (sparse_ls) { spls_algrad(x, grad, slot0); return; }
        if (desc.c_kind == BZ_C_SPARSE_AFFINE) {
            // two launches: rows of A (c(x), yhat, the penalty partials), rows of A' (A'yhat, grad f, the f partials);
            // the sparse quadratic f: a third in front, rows of Q (Q x -> FR_)
            if (sparse_f) spq_product(x, FR_.p, false, (int)SL_SCRATCH);
            slot_n[slot0 + 1] = spmv_yupd(x, cx_keep_, YU_.p, slot0 + 1);
            slot_n[slot0] = spmv_t_finish(x, grad, slot0);
            gather(slot0, 2, 0u, 2u);
            return;
        }
        if (desc.c_kind == BZ_C_DENSE_AFFINE && dense_fused_on()) {
            // one pass over A: c(x), yhat and the row-group partials of A'yhat (k_dense_fused), then the fold + f terms
            slot_n[slot0] = grid;
            dense_fused_launch(x, slot0 + 1);
            mv(df_groups_ + 2 + pstreams(true, false, false));
            launch(C_MISC, k_gemv_t_finish<T>, grid, (const T*)GT_.p, df_groups_, npad, x, P, grad, n, parts_.p, slot0);
            gather(slot0, 2, 0u, 2u);
            return;
        }
        if (desc.c_kind == BZ_C_DENSE_AFFINE) {
            // the two-kernel form: one pass over A for A x, one ny-length kernel, one pass over A for A' yupd, the finish
            // (x: nx elements — the x half of the lifted vector in the slack form, whose s half follows it)
            slot_n[slot0] = grid_x; slot_n[slot0 + 1] = grid_y;
            // dense f: its own products first (grad f -> DFX_ / Q x -> FR_ ; LeastSquares: <r, r> -> slot0, with its own count)
            if (dense_f) dense_f_eval(x, slot0, true);
            eval_c(x);                                                        // cx = A x - b
            if (cx_keep_) BZ_HIP(hipMemcpyAsync(cx_keep_, CX_.p, ny * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
            if (slack) {
                // w = (cx + mu y) - s, sum w^2/mu, yupd = y + (cx - s)/mu and dFxs[nx:] = -yupd in one pass
                mv(5 + 1 + (grad ? 1 : 0), ny); nm("k_algrad_slack_rows");
                launch(C_ALGRAD, k_algrad_slack_rows<T>, grid_y, (const T*)CX_.p, x + nx, (const T*)mu_.p, (const T*)muy_.p,
                       (const T*)ymul_.p, YU_.p, grad ? grad + nx : (T*)nullptr, ny, parts_.p, slot0 + 1);
            } else {
                mv(2 + pstreams(false, true, false), ny);
                launch(C_MISC, k_yupd<T>, grid_y, (const T*)CX_.p, P, YU_.p, ny, parts_.p, slot0 + 1);
            }
            gemv_cols(A_.p, ny, nx, YU_.p, rows_per_chunk, nrowchunks, GT_.p, npadx);      // jtv = A' yupd (row-chunk partials)
            if (dense_f) {
                // dlx = dfx + jtv with the dense f's gradient (k_algrad_elem's modes 1 and 2)
                const bool ls = desc.f_kind == BZ_F_LEAST_SQUARES;
                mv(nrowchunks + 3 + (ls ? 0 : 1), nx); nm("k_gemv_t_finish_ext");
                launch(C_MISC, k_gemv_t_finish_ext<T>, grid_x, (const T*)GT_.p, nrowchunks, npadx, x, P, ls ? 1 : 2,
                       ls ? (const T*)DFX_.p : (const T*)FR_.p, grad, nx, parts_.p, slot0);
            } else if (x_replicated) {
                // this rank's rows only: fold the chunks, sum over the ranks (rank order), then finish
                ElemParams<T> Pz = P;
                Pz.f_kind = BZ_F_ZERO;
                mv(nrowchunks + 2);
                launch(C_MISC, k_gemv_t_finish<T>, grid, (const T*)GT_.p, nrowchunks, npad, x, Pz, JL_.p, n, parts_.p,
                       (int)SL_SCRATCH);
                const T* chunks = allreduce_partials();
                mv(ctx->nranks + 2 + pstreams(true, false, false));
                launch(C_MISC, k_gemv_t_finish<T>, grid, chunks, ctx->nranks, npad, x, P, grad, n, parts_.p, slot0);
            } else {
                mv(nrowchunks + 2 + pstreams(true, false, false), nx);
                launch(C_MISC, k_gemv_t_finish<T>, grid_x, (const T*)GT_.p, nrowchunks, npadx, x, P, grad, nx, parts_.p, slot0);
            }
            gather(slot0, 2, 0u, 2u);         // slot0: f terms (x-space) ; slot0 + 1: penalty terms (this rank's rows)
            return;
        }
        if (sparse_f && spq_fused_on()) {
            // c = Identity: one launch over the rows of Q
            slot_n[slot0] = slot_n[slot0 + 1] = spq_algrad(x, grad, slot0);
            gather(slot0, 2, 0u);
            return;
        }
        slot_n[slot0] = slot_n[slot0 + 1] = grid;
        if (slack) {
            slot_n[slot0] = slot_n[slot0 + 1] = grid_y;
            mv(2 + pstreams(true, false, false) + 3 + 2, nx);
            launch(C_ALGRAD, k_algrad_slack_elem<T>, grid_y, x, P, (const T*)ymul_.p, grad, nx, parts_.p, slot0);
            gather(slot0, 2, 0u);
            return;
        }
        if (sparse_f) {
            // the two-launch form: Q x -> FR_, then the element-wise kernel in its mode 2
            spq_product(x, FR_.p, false, (int)SL_SCRATCH);
            mv(4 + pstreams(false, true, false));
            launch(C_ALGRAD, k_algrad_elem<T>, grid, x, P, grad, n, parts_.p, slot0, 2, (const T*)FR_.p);
        } else if (dense_f) {
            dense_f_eval(x, slot0, true);
            if (desc.f_kind == BZ_F_LEAST_SQUARES)
                { mv(3 + pstreams(false, true, false)); launch(C_ALGRAD, k_algrad_elem<T>, grid, x, P, grad, n, parts_.p, slot0, 1, (const T*)DFX_.p); }
            else
                { mv(4 + pstreams(false, true, false)); launch(C_ALGRAD, k_algrad_elem<T>, grid, x, P, grad, n, parts_.p, slot0, 2, (const T*)FR_.p); }
        } else if (desc.f_kind == BZ_F_STENCIL5) {
            mv(3 + pstreams(false, true, false));      // x (its north / south / west / east re-reads are cache hits), b, grad
            launch(C_ALGRAD, k_algrad_stencil<T>, grid, x, P, (int64_t)desc.f_grid_nx, (int64_t)desc.f_grid_ny, 0,
                   grad, n, parts_.p, slot0, halo_exchange(x));
        } else {
            mv(2 + pstreams(true, true, false));
            launch(C_ALGRAD, k_algrad_elem<T>, grid, x, P, grad, n, parts_.p, slot0, 0, (const T*)nullptr);
        }
        gather(slot0, 2, 0u);
    }
    // f(x) alone (alps.jl:39): partial sums -> slot0
    void fvalue(const T* x, int slot0) {
        if (generic_) {      // f(x) through the gradient callback (the reference's generic f(x) needs no more)
            copy_out(hx_.data(), x, n);
            fill_slot(slot0, cb_f_gradient(hx_.data(), hdfx_.data(), n));
            return;
        }
        slot_n[slot0] = grid;
        if (slack) {      // f on the x part only
            slot_n[slot0] = grid_x;
            if (dense_f) {
                dense_f_eval(x, slot0, false);
                if (desc.f_kind == BZ_F_QUADRATIC)
                    { mv(3, nx); launch(C_MISC, k_fvalue_elem<T>, grid_x, x, P, nx, parts_.p, slot0, (const T*)FR_.p); }
            } else {
                mv(1 + pstreams(true, false, false), nx);
                launch(C_MISC, k_fvalue_elem<T>, grid_x, x, P, nx, parts_.p, slot0, (const T*)nullptr);
            }
            gather(slot0, 1, 0u);
            return;
        }
        if (sparse_ls) {
            slot_n[slot0] = spls_residual(x, nullptr, slot0);               // f(x) from the rows of A_f, r not kept
        } else if (sparse_f) {
            if (cenv_.spq_fused) {
                slot_n[slot0] = spq_product(x, nullptr, true, slot0);       // f(x) from the rows of Q, Q x not kept
            } else {
                spq_product(x, FR_.p, false, (int)SL_SCRATCH);
                mv(3); launch(C_MISC, k_fvalue_elem<T>, grid, x, P, n, parts_.p, slot0, (const T*)FR_.p);
            }
        } else if (dense_f) {
            dense_f_eval(x, slot0, false);
            if (desc.f_kind == BZ_F_QUADRATIC)
                { mv(3); launch(C_MISC, k_fvalue_elem<T>, grid, x, P, n, parts_.p, slot0, (const T*)FR_.p); }
        } else if (desc.f_kind == BZ_F_STENCIL5) {
            mv(2);
            launch(C_MISC, k_algrad_stencil<T>, grid, x, P, (int64_t)desc.f_grid_nx, (int64_t)desc.f_grid_ny, 1,
                   (T*)nullptr, n, parts_.p, slot0, halo_exchange(x));
        } else {
            mv(1 + pstreams(true, false, false));
            launch(C_MISC, k_fvalue_elem<T>, grid, x, P, n, parts_.p, slot0, (const T*)nullptr);
        }
        gather(slot0, 1, 0u);
    }

    // AugLagUpdate!(al, mu, y)  (auglagfun.jl:91-101) on the device copies mu_, ymul_ ; safeguard: the dual
    // safeguard of alps.jl:62 applied to y first, in the same pass
    int uni_ = 0;                            // P.uni as the last update found it: 1 uniform penalties, 2 and zero multipliers
    void aug_lag_update(bool safeguard = false) {
        // Uniform penalties / zero multipliers (this rank's part of them): the one-pass kernel then takes mu as a
        // number and does not stream mu (nor mu*y).  alps.jl:42 gives every constraint the same mu when c(x0) is
        // in D, alps.jl:97 scales them alike, and y0 = 0 holds through the first subproblem — the longest one.
        uni_ = 0;
        const int uni_env = read_uni_knob();
        const bool probe = uni_env && (fused_family() >= 0 || (slack && !lp_g) ||
                                       (desc.f_kind == BZ_F_STENCIL5 && desc.c_kind == BZ_C_IDENTITY && !slack && !lp_g && !group_g));
        for (int k = 0; k < 3; ++k) slot_n[SL_GP + k] = grid_y;
        slot_n[SL_OUTER] = slot_n[SL_OUTER + 1] = grid_y;
        mv(3 + (safeguard ? 1 : 0), ny);
        launch(C_MISC, k_muy<T>, grid_y, (const T*)mu_.p, ymul_.p, muy_.p, ny, parts_.p, (int)SL_OUTER,
               safeguard ? 1 : 0, probe ? (int)SL_GP : -1);
        gather(SL_OUTER, 2, 2u, 3u);
        std::vector<double> v, u;
        if (probe && !ctx->multi()) {
            // one read-back for both groups; the probe's slots are this rank's own (no exchange: every form of
            // the kernel gives the same bits)
            auto a5 = collect({SL_OUTER, SL_OUTER + 1, SL_GP, SL_GP + 1, SL_GP + 2}, 2u | (7u << 2));
            v = {a5[0], a5[1]}; u = {a5[2], a5[3], a5[4]};
        } else {
            v = collect({SL_OUTER, SL_OUTER + 1}, 2u);
            if (probe) {
                CollectArgs a;
                a.n = 3; a.maxmask = 7u;
                for (int k = 0; k < 3; ++k) a.src[k] = ScalarSrc{parts_.p + (size_t)(SL_GP + k) * PSTRIDE, grid_y, 1};
                u = collect_run(a);
            }
        }
        if (v[1] > 0.0) throw Error(BZ_ERR_MU, "parameters `mu` must be positive");
        musqy = T(0.5) * T(v[0]);
        if (generic_) { copy_out(hmu_.data(), mu_.p, ny); copy_out(hmuy_.data(), muy_.p, ny); }
        if (probe && u[1] == 0.0 && u[0] > 0.0) {
            uni_ = (u[2] == 0.0 && uni_env >= 2) ? 2 : 1;
            P.mu_uniform = (T)u[0];
        }
        P.uni = uni_;      // every kernel that takes the penalties through load_params takes them as numbers then
    }
    // the oracle family of the iterate-history one-pass kernel (fam_code, bz_kernels.h), or -1: c = Identity, an
    // element-wise f, any element-wise g but the Newton / L0 kinds, any D
    int fused_family() const {
        if (desc.c_kind != BZ_C_IDENTITY || slack || ny != n || lp_g || group_g) return -1;
        if (P.lambda_vec()) return -1;      // (a per-element lambda: no family for it, the stored-pair forms)
        if (enet_g) return -1;              // (the elastic net, with weights or without: the same)
        int fk, gk, dk;
        switch (desc.f_kind) {
        case BZ_F_ZERO: fk = FAM_F_ZERO; break;
        case BZ_F_DIAG_QUADRATIC: fk = FAM_F_DIAG; break;
        default: return -1;
        }
        switch (desc.g_kind) {
        case BZ_G_ZERO: gk = FAM_G_ZERO; break;
        case BZ_G_NORM_L1: gk = FAM_G_L1; break;
        case BZ_G_NORM_L1_NONNEG: gk = FAM_G_L1NONNEG; break;
        case BZ_G_NORM_L1_BOX: gk = FAM_G_L1BOX; break;
        case BZ_G_IND_BOX: gk = (P.g_lo_vec || P.g_hi_vec) ? FAM_G_INDBOX_VEC : FAM_G_INDBOX; break;
        default: return -1;
        }
        switch (desc.D_kind) {
        case BZ_D_ZERO: dk = FAM_D_ZERO; break;
        case BZ_D_FREE: dk = FAM_D_FREE; break;
        case BZ_D_BOX: dk = (P.D_lo_vec || P.D_hi_vec) ? FAM_D_BOX_VEC : FAM_D_BOX; break;
        case BZ_D_VC_PAIRS: dk = FAM_D_VC; break;
        case BZ_D_CC_PAIRS: dk = FAM_D_CC; break;
        case BZ_D_EITHEROR_PAIRS: dk = FAM_D_EITHEROR; break;
        case BZ_D_XOR_PAIRS: dk = FAM_D_XOR; break;
        default: return -1;
        }
        return fam_code(fk, gk, dk);
    }

    // --------------------------------------------------------------- L-BFGS
    void alloc_history() {
        if ((int)S_.size() == state_.lbfgs.M + 1) return;
        S_ = std::vector<DBuf<T>>(state_.lbfgs.M + 1);
        Y_ = std::vector<DBuf<T>>(state_.lbfgs.M + 1);
        for (int i = 0; i <= state_.lbfgs.M; ++i) { S_[i].alloc(vcap); Y_[i].alloc(vcap); }
        if (affine_ok_) {
            AS_ = std::vector<DBuf<T>>(state_.lbfgs.M + 1); AY_ = std::vector<DBuf<T>>(state_.lbfgs.M + 1);
            GS_ = std::vector<DBuf<T>>(state_.lbfgs.M + 1); GY_ = std::vector<DBuf<T>>(state_.lbfgs.M + 1);
            for (int i = 0; i <= state_.lbfgs.M; ++i) { AS_[i].alloc(ny); AY_[i].alloc(ny); GS_[i].alloc(vcap); GY_[i].alloc(vcap); }
        }
    }
    void lbfgs_reset() {                 // reset!(H): currmem = curridx = 0, H = 1
        if (dir_kind_ == BZ_DIR_BROYDEN) broyden_reset();
        state_.lbfgs.reset();
    }
    CompactVecs<T, CM> compact_vecs() const {      // logical (oldest first) view of the physical ring
        CompactVecs<T, CM> V;
        std::memset(&V, 0, sizeof(V));
        V.m = (int)state_.lbfgs.order.size();
        for (int i = 0; i < V.m; ++i) { V.S[i] = S_[state_.lbfgs.order[V.m - 1 - i]].p; V.Y[i] = Y_[state_.lbfgs.order[V.m - 1 - i]].p; }
        return V;
    }
    // coefficient block for the kernels that apply the operator.  p = S'(-res), w = Y'(-res) normally came
    // back with the previous iteration's scalars; otherwise (the accepted trial was not the fused one)
    // they take their own pass and read-back
    CompactCoef<CM> compact_prepare(const CompactVecs<T, CM>& V) {
        const int m = V.m;
        if (m == 0) {
            for (int i = 0; i < CM; ++i) { state_.lbfgs.hp[i] = 0.0; state_.lbfgs.hw[i] = 0.0; }
            state_.lbfgs.pw_valid = true;
        }
        if (!state_.lbfgs.pw_valid) {
            for (int k = 0; k < 2 * CM; ++k) slot_n[SL_GP + k] = grid;
            mv(2 * m + 1);
            launch(C_DOT, k_gram_dots<T, CM>, grid, V, (const T*)RES_[rc].p, n, parts_.p, (int)SL_GP);
            gather(SL_GP, 2 * CM, 0u);
            auto pv = collect_range(SL_GP, 2 * CM, 0u);
            for (int i = 0; i < CM; ++i) { state_.lbfgs.hp[i] = i < m ? pv[i] : 0.0; state_.lbfgs.hw[i] = i < m ? pv[CM + i] : 0.0; }
            state_.lbfgs.pw_valid = true;
        }
        CompactCoef<CM> C;
        std::memset(&C, 0, sizeof(C));
        state_.lbfgs.coefficients(dir_kind_ == BZ_DIR_ANDERSON, C.H0, C.u1, C.u2h);
        return C;
    }

    // d = H(-res) up to the last axpy, which the caller fuses with what follows
    // same result through the persistent kernel (one launch, d register-resident)
    TailArgs<T> two_loop_persist() {
        TailArgs<T> t;
        std::memset(&t, 0, sizeof(t));
        t.alphas = alphas_.p;
        const int m = (int)state_.lbfgs.order.size();
        PersistArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        a.res = RES_[rc].p;
        for (int j = 0; j < m; ++j) { a.S[j] = S_[state_.lbfgs.order[j]].p; a.Y[j] = Y_[state_.lbfgs.order[j]].p; a.ys[j] = state_.lbfgs.ys[state_.lbfgs.order[j]]; }
        a.H = state_.lbfgs.H; a.m = m; a.d_out = D_.p; a.n = n; a.parts = parts_.p; a.alphas = alphas_.p;
        a.counter = pcounter_.p; a.base = pbase + (env_.test_persist_timeout ? 1ull : 0ull); a.timeout = ptimeout_dev_;
        a.abort_flag = pgflag_.p + 1;
        a.slot_loop1 = SL_LOOP1; a.slot_loop2 = SL_LOOP2;
        a.nb = persist_blocks();
        const bool multi = ctx->nranks > 1;
        const int nphases = 2 * m - 1 + (multi ? 1 : 0);
        a.nranks = ctx->nranks; a.rank = ctx->rank; a.pseq = ctx->pseq + 1;
        if (multi) {
            a.mbox_local = (P2PWords*)ctx->mbox_local;
            for (int r = 0; r < ctx->nranks; ++r) a.mbox_peer[r] = (P2PWords*)ctx->mbox_peer[r];
            a.gtot = pglobal_.p; a.gflag = pgflag_.p; a.final_tot = pglobal_.p + 2;
            ctx->pseq += nphases;
        }
        pbase += (unsigned long long)nphases * a.nb;
        mv(4 * m, vcap);
        form_[C_PERSIST] = "k_twoloop_persist<KR=" + std::to_string(persist_kr) + ">";
        switch (persist_kr) {
#define BZ_KR_CASE(K) case K: launch_persist(k_twoloop_persist<T, K>, a); break;
        BZ_KR_CASE(1) BZ_KR_CASE(2) BZ_KR_CASE(3) BZ_KR_CASE(4) BZ_KR_CASE(5) BZ_KR_CASE(6) BZ_KR_CASE(7) BZ_KR_CASE(8)
        BZ_KR_CASE(10) BZ_KR_CASE(12) BZ_KR_CASE(14) BZ_KR_CASE(16) BZ_KR_CASE(20) BZ_KR_CASE(24) BZ_KR_CASE(28)
        BZ_KR_CASE(32) BZ_KR_CASE(36) BZ_KR_CASE(40) BZ_KR_CASE(44) BZ_KR_CASE(48)
#undef BZ_KR_CASE
        default: throw Error(BZ_ERR_STATE, "persistent two-loop: no instantiation for this size");
        }
        slot_n[SL_LOOP2 + 0] = a.nb;
        t.in = D_.p; t.sgn = T(1); t.v = S_[state_.lbfgs.order[0]].p; t.mode = 1; t.j = 0; t.apply_H = 0; t.H = T(1);
        t.src = multi ? ScalarSrc{pglobal_.p + 2, 1, 1} : src(SL_LOOP2 + 0);
        t.ys = state_.lbfgs.ys[state_.lbfgs.order[0]];
        return t;
    }
    int persist_blocks() const { return pblocks; }
    static int persist_occupancy(int kr) {
        int nb = 0;
        hipError_t e = hipErrorInvalidValue;
        switch (kr) {
#define BZ_KR_CASE(K) case K: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)k_twoloop_persist<T, K>, PBLOCK, 0); break;
        BZ_KR_CASE(1) BZ_KR_CASE(2) BZ_KR_CASE(3) BZ_KR_CASE(4) BZ_KR_CASE(5) BZ_KR_CASE(6) BZ_KR_CASE(7) BZ_KR_CASE(8)
        BZ_KR_CASE(10) BZ_KR_CASE(12) BZ_KR_CASE(14) BZ_KR_CASE(16) BZ_KR_CASE(20) BZ_KR_CASE(24) BZ_KR_CASE(28)
        BZ_KR_CASE(32) BZ_KR_CASE(36) BZ_KR_CASE(40) BZ_KR_CASE(44) BZ_KR_CASE(48)
#undef BZ_KR_CASE
        default: break;
        }
        if (e != hipSuccess) { (void)hipGetLastError(); return 0; }
        return nb;
    }
    // register packs per thread: the smallest instantiated count >= the need (rounds past the need
    // stream zero padding, so the steps are finer where the relative waste would be larger)
    static int persist_round_kr(int kneed) {
        static const int ks[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 36, 40, 44, 48};
        for (int k : ks) if (k >= kneed) return k;
        return 0;
    }
    template <class K> void launch_persist(K kernel, const PersistArgs<T>& a) {
        ProfRec r{C_PERSIST, nullptr, nullptr, 0.0};
        const bool prof_on = prof_pick(C_PERSIST);
        account(C_PERSIST, prof_on ? &r : nullptr);
        if (prof_on) {
            r.a = get_event(); r.b = get_event();
            hipExtLaunchKernelGGL(kernel, dim3(a.nb), dim3(PBLOCK), 0, ctx->stream, r.a, r.b, 0, a);
            prof_recs.push_back(r);
        } else {
            hipLaunchKernelGGL(kernel, dim3(a.nb), dim3(PBLOCK), 0, ctx->stream, a);
        }
        BZ_HIP(hipGetLastError());
    }

    TailArgs<T> two_loop() {
        TailArgs<T> t;
        std::memset(&t, 0, sizeof(t));
        t.alphas = alphas_.p;
        const int m = (int)state_.lbfgs.order.size();
        slot_n[SL_LOOP2 + 0] = grid;
        const T* res = RES_[rc].p;
        if (m == 0) {
            t.in = res; t.v = nullptr; t.sgn = T(-1); t.mode = 2; t.apply_H = 1; t.H = state_.lbfgs.H;
            t.src = ScalarSrc{parts_.p, 0, 1}; t.ys = T(1);
            return t;
        }
        mv(2);
        launch(C_DOT, k_dot<T>, grid, (const T*)S_[state_.lbfgs.order[0]].p, res, T(-1), n, parts_.p, SL_LOOP1 + 0);
        gather(SL_LOOP1 + 0, 1, 0u);
        for (int j = 0; j + 1 < m; ++j) {        // loop 1: d -= alpha_j y_j ; <s_{j+1}, d>
            TailArgs<T> a = t;
            a.in = (j == 0) ? res : (const T*)D_.p; a.sgn = (j == 0) ? T(-1) : T(1);
            a.v = Y_[state_.lbfgs.order[j]].p; a.mode = 0; a.j = j; a.apply_H = 0; a.H = T(1);
            a.src = src(SL_LOOP1 + j); a.ys = state_.lbfgs.ys[state_.lbfgs.order[j]];
            mv(4); nm("k_axpy_dot");
            launch(C_TWOLOOP, k_axpy_dot<T>, grid, a, (const T*)S_[state_.lbfgs.order[j + 1]].p, (const T*)nullptr,
                   D_.p, n, parts_.p, SL_LOOP1 + j + 1);
            gather(SL_LOOP1 + j + 1, 1, 0u);
        }
        {                                          // d = H (d - alpha_{m-1} y_{m-1}) ; <y_{m-1}, d>
            TailArgs<T> a = t;
            const int j = m - 1;
            a.in = (m == 1) ? res : (const T*)D_.p; a.sgn = (m == 1) ? T(-1) : T(1);
            a.v = Y_[state_.lbfgs.order[j]].p; a.mode = 0; a.j = j; a.apply_H = 1; a.H = state_.lbfgs.H;
            a.src = src(SL_LOOP1 + j); a.ys = state_.lbfgs.ys[state_.lbfgs.order[j]];
            mv(3);
            launch(C_TWOLOOP, k_axpy_dot<T>, grid, a, (const T*)Y_[state_.lbfgs.order[j]].p, (const T*)nullptr, D_.p,
                   n, parts_.p, SL_LOOP2 + j);
            gather(SL_LOOP2 + j, 1, 0u);
        }
        for (int j = m - 1; j >= 1; --j) {         // loop 2: d += (alpha_j - beta_j) s_j ; <y_{j-1}, d>
            TailArgs<T> a = t;
            a.in = D_.p; a.sgn = T(1); a.v = S_[state_.lbfgs.order[j]].p; a.mode = 1; a.j = j; a.apply_H = 0;
            a.H = T(1); a.src = src(SL_LOOP2 + j); a.ys = state_.lbfgs.ys[state_.lbfgs.order[j]];
            mv(4);
            launch(C_TWOLOOP, k_axpy_dot<T>, grid, a, (const T*)Y_[state_.lbfgs.order[j - 1]].p, (const T*)nullptr,
                   D_.p, n, parts_.p, SL_LOOP2 + j - 1);
            gather(SL_LOOP2 + j - 1, 1, 0u);
        }
        t.in = D_.p; t.sgn = T(1); t.v = S_[state_.lbfgs.order[0]].p; t.mode = 1; t.j = 0; t.apply_H = 0; t.H = T(1);
        t.src = src(SL_LOOP2 + 0); t.ys = state_.lbfgs.ys[state_.lbfgs.order[0]];
        return t;
    }

    // ------------------------------------------------ Base.iterate(iter)  (k = 1)
    void begin_dev(const bz_panoc_opts& o, const T* x0_dev) {
        try {
            begin_impl(o, x0_dev);
        } catch (const DenseFusedTimeout&) {
            // (the start of a solve writes nothing it does not write again: once more, in the two-kernel form)
            if (ctx->nranks > 1) throw;
            BZ_HIP(hipStreamSynchronize(ctx->stream));
            *ptimeout_ = 0;
            std::fprintf(stderr, "Warning: the one-pass dense kernel timed out (is the GPU shared?); using the two-kernel form\n");
            begin_impl(o, X_[0].p);
        }
    }
    // which forms a solve takes (begin_impl): the one-pass kernels, the stencil fast path, the affine images, the compact
    // representation, the persistent two-loop kernel
    void select_paths(const bz_panoc_opts& o) {
        // (the slack form of ALS too: x_i couples with s_i only — k_fused_slack; no pairwise D there, it needs the partner)
        fused_ok = o.fuse && desc.c_kind == BZ_C_IDENTITY && !lp_g && !group_g && (!slack || desc.D_kind < BZ_D_VC_PAIRS) &&
                   (desc.f_kind == BZ_F_ZERO || desc.f_kind == BZ_F_DIAG_QUADRATIC);
        // auto: the compact representation where it makes the whole iteration one pass (the fused separable
        // path, memory within its capacity), the two-loop recursion everywhere else
        // (... and the stencil path: x_d, k_stencil_fb, k_stencil_update_c with ONE reduction phase per iteration
        // instead of the persistent two-loop kernel's 2m - 1 grid barriers, or 2m + 1 exchanges when sharded)
        stencil_fast_ = desc.f_kind == BZ_F_STENCIL5 && o.fuse && !lp_g && !group_g && !slack;
        if (o.affine_refresh < 0) throw Error(BZ_ERR_ARG, "affine_refresh must be >= 0");
        aff_refresh_ = o.affine_refresh;
        aff_track_ = affine_ok_ && aff_refresh_ > 0 && o.lbfgs_compact != 0 && state_.lbfgs.M >= 1 && state_.lbfgs.M <= CM && dir_kind_ == BZ_DIR_LBFGS;
        compact_ok = state_.lbfgs.M >= 1 && (o.lbfgs_compact == 1 || dir_kind_ == BZ_DIR_ANDERSON ||
                                (o.lbfgs_compact == 2 && (fused_ok || stencil_fast_ || aff_track_) && state_.lbfgs.M <= CM));
        // persistent two-loop: d must fit the register files (<= 40 packs per thread, one 512-thread
        // block per CU) and the vector must be long enough for 2m-1 grid barriers to beat 2m launches;
        // with several ranks the phases need the p2p mailboxes (RCCL cannot be called from a kernel)
        persist_ok = o.persist && (!ctx->multi() || ctx->p2p_on) && persist_kr > 0 && n >= env_.persist_min_n && !x_replicated &&
                     !persist_broken_;
        if (ctx->nranks > 1 && !ctx->multi())
            throw Error(BZ_ERR_STATE, "nranks > 1 needs an RCCL communicator or connected p2p mailboxes");
        if (ctx->nranks > 1 && o.persist && state_.lbfgs.M >= 1) {
            // the shards may straddle a threshold (length, register budget): the phases of the persistent kernel
            // and the exchanges of the kernel chain do not talk to each other, so all ranks must take the same
            // form — the persistent one only if every rank can
            launch_b(C_MISC, k_fill_slot, 1, 64, parts_.p, (int)SL_AUX, persist_ok ? 0.0 : 1.0);
            slot_n[SL_AUX] = 1;
            gather(SL_AUX, 1, 1u);
            if (collect({SL_AUX}, 1u)[0] > 0.0) persist_ok = false;
        }
        // auto (lbfgs_compact = 2), one rank: wherever the two-loop would run as a CHAIN of 2m kernels (a vector beyond the
        // persistent kernel's register capacity — e.g. the lifted vector [x; s] of ALS at n = 1e7 — or too short for its
        // grid barriers) the compact form does the same work in two launches and 4m + 11 passes instead of 8m + 1
        // (ALS at n = 1e7: 741 against 519 it/s).  Several ranks keep the rule above: they must agree on one form.
        if (!compact_ok && o.lbfgs_compact == 2 && state_.lbfgs.M >= 1 && state_.lbfgs.M <= CM && dir_kind_ == BZ_DIR_LBFGS && !ctx->multi() && !persist_ok &&
            !generic_)
            compact_ok = true;
    }
    // the start of a solve (and the re-materialised z) in one element-wise pass: k_begin_lip, and k_begin_fb / k_zres_elem
    // unless g is an Lp power
    bool begin_lip_ok() const {
        return env_.fused_begin && desc.c_kind == BZ_C_IDENTITY && !slack && !dense_f &&
               (desc.f_kind == BZ_F_ZERO || desc.f_kind == BZ_F_DIAG_QUADRATIC);
    }
    bool begin_fb_ok() const { return begin_lip_ok() && !lp_g && !group_g; }
    void begin_impl(const bz_panoc_opts& o, const T* x0_dev) {
        env_ = BeginKnobs(ctx->nranks);
        opt = o;
        if (o.lbfgs_memory < 0 || o.lbfgs_memory > MAX_MEM)
            throw Error(BZ_ERR_ARG, "lbfgs_memory must be in 0..16 (0 = NoAcceleration)");
        if (o.max_backtracks < 1) throw Error(BZ_ERR_ARG, "max_backtracks must be >= 1");
        int M = o.lbfgs_memory;
        if (o.directions != BZ_DIR_LBFGS && o.directions != BZ_DIR_ANDERSON && o.directions != BZ_DIR_BROYDEN)
            throw Error(BZ_ERR_ARG, "unknown `directions`");
        dir_kind_ = o.directions;
        if (dir_kind_ == BZ_DIR_ANDERSON && (M < 1 || M > CM))
            throw Error(BZ_ERR_ARG, "AndersonAcceleration(n): 1 <= n <= 5");
        if (dir_kind_ == BZ_DIR_BROYDEN) {
            if (n > 4096) throw Error(BZ_ERR_UNSUPPORTED, "Broyden() keeps a dense n-by-n operator: n <= 4096");
            if (ctx->nranks > 1) throw Error(BZ_ERR_UNSUPPORTED, "Broyden() is not sharded");
            M = 0;                                   // no pair history: the operator is the matrix
            broyden_theta_bar_ = (T)o.broyden_theta_bar;
            if (!HB_.p) {
                HB_.alloc((size_t)n * n); BHy_.alloc(npad); BsH_.alloc(npad);
                plan_chunks(n, n, b_rpc_, b_nch_);
                if (GT_.n < (size_t)b_nch_ * npad) GT_.alloc((size_t)b_nch_ * npad);
            }
        }
        state_.lbfgs.reset_all(M);
        alloc_history();
        if (dir_kind_ == BZ_DIR_BROYDEN) broyden_reset();
        if (o.lbfgs_compact < 0 || o.lbfgs_compact > 2) throw Error(BZ_ERR_ARG, "lbfgs_compact must be 0, 1 or 2 (auto)");
        if (o.lbfgs_compact == 1 && M > CM) throw Error(BZ_ERR_ARG, "lbfgs_compact supports lbfgs_memory <= 5");
        alpha = (T)o.alpha; beta = (T)o.beta; min_gamma = (T)o.minimum_gamma;
        // Lf = nothing, gamma = Lf === nothing ? nothing : alpha / Lf, adaptive = gamma === nothing   (upstream's keywords)
        if (o.gamma < 0.0 || o.Lf < 0.0 || o.gamma != o.gamma || o.Lf != o.Lf) throw Error(BZ_ERR_ARG, "gamma and Lf must be >= 0 (0 = nothing)");
        if (o.adaptive < -1 || o.adaptive > 1) throw Error(BZ_ERR_ARG, "adaptive must be -1 (default), 0 or 1");
        gamma_given_ = o.gamma > 0.0 ? (T)o.gamma : (o.Lf > 0.0 ? alpha / (T)o.Lf : T(0));
        // (upstream tests `iter.gamma === nothing || iter.adaptive == true` at both halving sites: without a given step
        // size the estimate is always backtracked, whatever `adaptive` says)
        adaptive_ = !(gamma_given_ > T(0)) || o.adaptive == 1;
        select_paths(o);
        state_.aff_count = 0; state_.n_affine = 0; state_.n_affine_blends = 0; n_gated_ = 0; n_gate_aborts_ = 0; n_dense_onepass_ = 0;
        t_begin = std::chrono::steady_clock::now();
        cnt_.k = 1; cnt_.n_grad = cnt_.n_prox = cnt_.n_bt = cnt_.n_halv = cnt_.n_fused = cnt_.n_skips = 0;
        last_nbt = 0; last_fused = false; tau = T(0); last_ys = T(0); state_.fbe_last = T(0);
        xc = 0; rc = 0; zc = 0; state_.z_valid = true; xr_run_ = 0; sy_stale_ = false; state_.res_valid = true;
        // BZ_GATE: 0 off; non-zero (default) the early launch queues behind the read-back on the solver's stream
        // Several ranks: off unless asked for (BZ_GATE=1).  A launch that misses its gate cannot be redone there (the peers
        // have consumed this rank's scalars: BZ_ERR_COMM), and gated launches on distinct devices have never run on
        // hardware — bench.py asks for them after checking, on the node it runs on, that they reproduce the plain launches.
        gate_env_ = env_.gate;
        // a resident launch polling at its gate holds its CUs: with another tenant on the GPU (a rank of this very job in
        // a one-GPU rehearsal, or whoever made an earlier launch of this problem miss its gate) the two starve each other
        if (ctx->shared_device || gate_broken_) gate_env_ = 0;
        gate_sabotage_ = env_.test_gate_timeout;
        if (gate_env_ && fused_ok) gate_alloc();      // (pinned record, device copy: not inside an iteration)
        gate_abort();
        if (x0_dev != X_[0].p)
            BZ_HIP(hipMemcpyAsync(X_[0].p, x0_dev, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        const T eps = std::numeric_limits<T>::epsilon();
        T* x = X_[xc].p;
        // grad_f_x, f_x = gradient(f, x)
        if (begin_lip_ok()) {
            // gradient at x and the Lipschitz estimate in one pass (k_begin_lip)
            slot_n[SL_FXD] = slot_n[SL_FXD + 1] = grid;
            mv(2 + pstreams(true, true, false));
            launch(C_ALGRAD, k_begin_lip<T>, grid, (const T*)x, P, GX_.p, n, parts_.p, (int)SL_FXD, (int)SL_AUX);
            gather(SL_FXD, 2, 0u);
            cnt_.n_grad += 2; state_.gx_valid = true;
        } else {
            if (aff_track_) cx_keep_ = CXS_.p;
            algrad(x, GX_.p, SL_FXD); ++cnt_.n_grad; state_.gx_valid = true;
            cx_keep_ = nullptr;
            if (!(gamma_given_ > T(0))) {
                // gamma = alpha / lower_bound_smoothness_constant(f, I, x, grad_f_x)
                mv(2);
                launch(C_MISC, k_add_scalar<T>, grid, (const T*)x, T(1), TMP_.p, n);
                algrad(TMP_.p, GZ_.p, SL_FZ); ++cnt_.n_grad;
                mv(4);
                launch(C_MISC, k_diff_ss2<T>, grid, (const T*)GZ_.p, (const T*)GX_.p, (const T*)TMP_.p, (const T*)x, n,
                       parts_.p, (int)SL_AUX);
            }
        }
        if (gamma_given_ > T(0)) {
            // gamma given (or Lf): no Lipschitz estimate; the one-pass start above computed it for free and it is ignored
            auto v = collect({SL_FXD, SL_PXD}, 0u);
            state_.f_x = al_value(v[0], v[1]);
            state_.gamma = gamma_given_;
        } else {
            slot_n[SL_AUX] = slot_n[SL_AUX + 1] = grid;
            gather(SL_AUX, 2, 0u);
            auto v = collect({SL_FXD, SL_PXD, SL_AUX, SL_AUX + 1}, 0u);
            state_.f_x = al_value(v[0], v[1]);
            const T Lest = std::sqrt(T(v[2])) / std::sqrt(T(v[3]));
            state_.gamma = alpha / Lest;
        }
        // y = x - gamma grad ; z, g_z = prox(g, y, gamma) ; res = x - z ; backtrack_stepsize!
        T f_z = T(0);
        const bool fused_fb = begin_fb_ok();
        double stop0 = 0.0;
        for (;;) {
            std::vector<double> v;
            if (fused_fb) {
                // FB step, gradient at z and stop norm in one pass (k_begin_fb)
                for (int k = 0; k < 8; ++k) slot_n[SL_GSUM + k] = grid;
                mv(4 + pstreams(true, true, true));
                launch(C_FB, k_begin_fb<T>, grid, (const T*)x, (const T*)GX_.p, state_.gamma, P, Z_[zc].p, RES_[rc].p, n,
                       parts_.p, (int)SL_GSUM);
                gather(SL_GSUM, 8, 1u << 7);
                ++cnt_.n_prox; ++cnt_.n_grad; state_.gz_valid = false;
                v = collect({SL_GSUM, SL_DOT, SL_SS, SL_FZ, SL_PZ, SL_STOP}, 1u << 5);
                stop0 = v[5];
            } else {
                fbstep(x, GX_.p, state_.gamma, Z_[zc].p, RES_[rc].p, SL_GSUM);
                gather(SL_GSUM, 3, 0u);
                ++cnt_.n_prox;
                if (aff_track_) cx_keep_ = CZS_.p;
                algrad(Z_[zc].p, GZ_.p, SL_FZ); ++cnt_.n_grad; state_.gz_valid = true;
                cx_keep_ = nullptr;
                v = collect({SL_GSUM, SL_DOT, SL_SS, SL_FZ, SL_PZ}, 0u);
            }
            state_.g_z = g_value(v[0]); state_.dot_gr = T(v[1]); state_.ss_res = T(v[2]);
            f_z = al_value(v[3], v[4]); state_.fraw_last = f_value(v[3]); state_.f_z_al = f_z;
            const T nr = std::sqrt(state_.ss_res);
            const T f_z_upp = state_.f_x - state_.dot_gr + ((alpha / state_.gamma) / T(2)) * (nr * nr);
            const T tol = T(10) * eps * (T(1) + std::abs(f_z));
            // (upstream: `if (iter.gamma === nothing || iter.adaptive == true)` backtrack_stepsize!)
            // (an infinite gamma — a zero Lipschitz estimate: grad F(x + 1) = grad F(x), e.g. f = Zero in the slack form — cannot be
            // halved: the reference's loop compares NaNs there and leaves; here f(z) may come out +inf, so say it explicitly)
            if (adaptive_ && std::isfinite((double)state_.gamma) && f_z > f_z_upp + tol && state_.gamma >= min_gamma) {
                state_.gamma = state_.gamma / T(2); ++cnt_.n_halv;
                continue;
            }
            break;
        }
        if (state_.gamma < min_gamma)
            std::fprintf(stderr, "Warning: stepsize `gamma` became too small (%g)\n", (double)state_.gamma);
        if (fused_fb) {
            stop_norm_ = stop0;
        } else {
            for (int k = 0; k < 3; ++k) slot_n[SL_YS + k] = grid;
            mv(4);
            launch(C_UPDATE, k_update<T>, grid, (const T*)x, (const T*)nullptr, (const T*)RES_[rc].p,
                   (const T*)nullptr, (const T*)GX_.p, (const T*)GZ_.p, state_.gamma, (T*)nullptr, (T*)nullptr, n,
                   parts_.p, (int)SL_YS);
            gather(SL_YS, 3, 4u);
            auto v = collect({SL_STOP}, 1u);
            stop_norm_ = v[0];
        }
        gring_[xc] = (double)state_.gamma;
        active = true;
    }

    void run_to_completion() {
        LoopGuard guard{this};
        for (;;) {
            const bool stop = should_stop();
            if (stop) gate_abort();              // (a pass pre-launched for an iteration that will not happen)
            if (opt.verbose && (stop || (opt.freq > 0 && cnt_.k % opt.freq == 0))) display();
            if (stop) break;
            more_coming_ = cnt_.k + 1 < opt.maxit;      // the solver's own loop: another iteration follows unless this one stops it
            step();
        }
    }

    void display() {
        ensure_z();
        mv(1);
        slot_n[SL_AUX] = grid;
        launch(C_MISC, k_absmax<T>, grid, (const T*)RES_[rc].p, n, parts_.p, (int)SL_AUX);
        gather(SL_AUX, 1, 1u);
        auto v = collect({SL_AUX}, 1u);
        std::printf("%5lld | %.3e | %.3e | %.3e\n", (long long)cnt_.k, (double)state_.gamma, v[0] / (double)state_.gamma,
                    (double)tau);
    }

    // ---------------------------------------- Base.iterate(iter, state)  (k += 1)
   public:
    // (leaving a library-run loop, normally or by an exception: no pass stays pre-launched at its gate, the flag that
    // allows pre-launching is down)
    struct LoopGuard {
        Solver* s;
        ~LoopGuard() {
            s->more_coming_ = false;
            s->gate_abort();
        }
    };
    void steps(int64_t k) override {
        LoopGuard guard{this};
        for (int64_t i = 0; i < k; ++i) {
            more_coming_ = i + 1 < k;            // (the caller asked for all k: the next pass may be launched early)
            step();
        }
    }
    void step() override {
        require_active();
        // Two things can make an iteration fail without having committed anything of the state, and both are reported
        // through the next read-back: a grid barrier of the persistent two-loop kernel that cannot complete (its
        // workgroups are not all resident: another stream or process holds CUs), and a pass pre-launched behind its gate
        // that gave up there (the host was descheduled for seconds, or the GPU has another tenant).  The iteration is
        // simply redone — with the kernel chain, without the gate — and the form that failed stays off for this
        // problem.  Whatever else goes wrong leaves with no launch waiting at a gate.
        const IterCounters sv = cnt_;
        const unsigned long long sv_pseq = ctx->pseq;
        auto restore = [&]() { cnt_ = sv; state_.gx_valid = false; state_.gz_valid = false; };
        // (a one-pass dense timeout is seen at a read-back of the iteration, possibly a later one than the first: by then the
        // attempt may have traded the image buffers, halved gamma, reset the memory and replaced the state's scalars)
        // (only the one-pass kernel reports such a timeout: other problems skip the snapshot)
        std::optional<IterState> sv_state;
        if (dense_fused_on()) sv_state = snapshot();
        try {
            try {
                step_impl();
            } catch (const GateTimeout&) {
                // (several ranks: the others have taken this rank's stale scalars for good ones — not recoverable here)
                if (ctx->nranks > 1) throw;
                gate_abort();              // (the pass launched early for the iteration after this one)
                BZ_HIP(hipStreamSynchronize(ctx->stream));
                *ptimeout_ = 0;
                restore();
                gate_broken_ = true; gate_env_ = 0; ++n_gate_fallbacks_;
                std::fprintf(stderr, "Warning: a pre-launched pass timed out at its gate (is the GPU shared?); gated pre-launch is off for this problem\n");
                step_impl();
            } catch (const DenseFusedTimeout&) {
                // the one-pass dense kernel's workgroups wait for each other (k_dense_fused): with CUs held by somebody else a
                // row group can be partly resident — the two-kernel form from now on, and the iteration again
                if (ctx->nranks > 1) throw;
                gate_abort();
                BZ_HIP(hipStreamSynchronize(ctx->stream));
                *ptimeout_ = 0;
                if (!sv_state || (dir_kind_ == BZ_DIR_BROYDEN && cnt_.n_halv != sv.n_halv)) throw;      // (a halving resets Broyden's operator itself)
                restore();
                put_back(*sv_state);
                std::fprintf(stderr, "Warning: the one-pass dense kernel timed out (is the GPU shared?); using the two-kernel form\n");
                step_impl();
            } catch (const PersistTimeout&) {
                if (!persist_ok) throw;
                BZ_HIP(hipStreamSynchronize(ctx->stream));
                *ptimeout_ = 0;
                BZ_HIP(hipMemsetAsync(pcounter_.p, 0, PSHARDS * PSHARD_STRIDE * sizeof(unsigned long long), ctx->stream));
                BZ_HIP(hipMemsetAsync(pgflag_.p, 0, 2 * sizeof(unsigned long long), ctx->stream));
                BZ_HIP(hipStreamSynchronize(ctx->stream));
                pbase = 0; ctx->pseq = sv_pseq;
                restore();
                persist_ok = false; persist_broken_ = true; ++n_persist_fallbacks_;
                std::fprintf(stderr, "Warning: persistent two-loop kernel timed out at its grid barrier; using the kernel chain\n");
                step_impl();
            }
        } catch (...) {
            more_coming_ = false;
            gate_abort();
            throw;
        }
        if (!more_coming_) gate_abort();
    }
   private:
    // the affine-image buffers in the order of IterState::img
    std::array<DBuf<T>*, 8> image_bufs() { return {&GX_, &GXN_, &GZ_, &GZN_, &CXS_, &CXD_, &CZS_, &CZN_}; }
    IterState snapshot() {
        IterState sv = state_;
        const auto b = image_bufs();
        for (int i = 0; i < 8; ++i) sv.img[i] = ImageRef{b[i]->p, b[i]->n};
        return sv;
    }
    void put_back(const IterState& sv) {
        state_ = sv;
        const auto b = image_bufs();
        for (int i = 0; i < 8; ++i) { b[i]->p = sv.img[i].p; b[i]->n = sv.img[i].n; }
        cx_keep_ = nullptr;
        // without images the attempt wrote grad L at its trial points into GX_ and GZ_ themselves (the redo evaluates them)
        state_.gx_valid = aff_track_ && sv.gx_valid; state_.gz_valid = aff_track_ && sv.gz_valid;
    }
    // ---- one iteration (step_impl), stage by stage.  Iter holds what lives inside the iteration only: the state it changes
    // is in state_ and cnt_, which step() snapshots.
    static constexpr int NFC = 10 + 4 * CM + 2;                          // slots of k_fused_compact
    static_assert(SL_TRIAL + NFC <= SL_AUX, "k_fused_compact's slots overlap the next group");
    struct Iter {
        T nr0, FBE_x;                            // ||res|| and the FBE at the current state
        bool stencil_fast_now, use_compact;
        CompactVecs<T, CM> CV;                   // the direction: compact coefficients ...
        CompactCoef<CM> CC;
        TailArgs<T> tail;                        // ... or the last axpy of the two-loop recursion / Broyden
        int m_at_trial;
        int xp, xd, xb, rp, rn, zp, zn;          // rings: the state's x, x_d, the tau blend; res; z
        int xcur, nbt = 0;                       // the trial point (x_d or the blend) ; tau backtracks so far
        bool have_trial = false, fused_this = false, reset_this = false, sep_trial = false;
        bool img_trial = false;      // grad L (and f) at the trial point x + d are affine images, not evaluations
        bool z_skipped = false, res_skipped = false, gram_from_trial = false;
        bool tail_used = false; unsigned long long tail_ticket = 0;      // the trial's scalars come back through the ticket
        bool head_on = false, head_fb = false;   // cfg 4: k_dense_head serves this iteration ; ... and has made the FB step of its first trial
        bool state_imgs = false, halved_here = false;      // cfg 4: the state's images are valid ; gamma was halved inside this step
        // the step's last trial (k = max_backtracks) asked for a halving: the loop ends there, the trial is not repeated and
        // becomes the state with z, res and the pair formed with the gamma BEFORE the halving (gamma_res); whether that
        // trial was the first one-pass launch (z, res possibly not stored), and whether its pair lives in the iterate ring only
        bool halved_last = false, last_fused = false, last_ring = false;
        T gamma_res = T(0);
        // a backtracked trial point can go through the one-pass kernel too ("trial given" variant) when this iteration's
        // first trial did: that launch's plan and coefficients
        bool trial_ok = false; GatePlan trial_plan; CompactCoef<CM> trial_coef;
        double sep_p = 0.0, sep_w = 0.0;         // <s_new, -res>, <y_new, -res> as measured by a k_fused_sep trial
        double gsy[CM] = {0}, gyy[CM] = {0};
        double tp[CM] = {0}, tw[CM] = {0}, tpn = 0.0, twn = 0.0;      // next p, w as measured by the fused trial
        std::vector<double> v;                   // the accepted trial's scalars
        bool gen_gram = false;       // the generic trial just launched carried the compact form's products (k_update_c)
        int m_gram;                  // ... measured against a memory of this many pairs
    };
    void step_impl() {
        ++cnt_.k;
        Iter it;
        open_iteration(it);
        if (fused_ok && it.use_compact) trial_onepass(it);
        else if (fused_ok && !slack) trial_sep(it);
        else trial_chain(it);
        step_size_test(it);
        commit(it);
    }
    // the FBE at the current state, which paths apply, the direction d = H(-res) (all but the last axpy), the ring indices
    void open_iteration(Iter& it) {
        it.nr0 = std::sqrt(state_.ss_res);
        it.FBE_x = (state_.f_x - state_.dot_gr + ((alpha / state_.gamma) / T(2)) * (it.nr0 * it.nr0)) + state_.g_z;
        state_.fbe_last = it.FBE_x;
        // (headline family: the one-pass kernel also serves an EMPTY memory — d = H0 (-res), all coefficients zero —
        // so the first iteration of a solve is a 3..5-stream pass too instead of k_fused_sep's 12)
        // (the stencil fast path also serves a row-sharded grid: the halo rows of x_d and of z travel before the two
        // passes, and with the compact form the iteration has ONE scalar exchange — the 32 slots of k_stencil_update_c)
        it.stencil_fast_now = stencil_fast_ && (!ctx->multi() || (ctx->p2p_on && compact_ok));
        it.use_compact = compact_ok && (!state_.lbfgs.order.empty() || (fused_ok && fused_family() >= 0) || it.stencil_fast_now || aff_track_);
        const bool use_persist = persist_ok && !state_.lbfgs.order.empty() && !it.use_compact;
        if (it.use_compact) { it.CV = compact_vecs(); it.CC = compact_prepare(it.CV); std::memset(&it.tail, 0, sizeof(it.tail)); }
        else if (dir_kind_ == BZ_DIR_BROYDEN) { if (!state_.res_valid) ensure_z(); it.tail = broyden_dir(); }
        else it.tail = use_persist ? two_loop_persist() : two_loop();
        it.m_at_trial = it.m_gram = (int)state_.lbfgs.order.size();
        tau = T(1);
        it.xp = xc; it.xd = (xc + 1) % NXR; it.xb = (xc + 2) % NXR;
        it.rp = rc; it.rn = (rc + 1) % NRR; it.zp = zc; it.zn = 1 - zc;
        it.xcur = it.xd;
    }

    // ---- the first trial, one function per path
    // one-pass kernels with the compact form: x_d, the FB step, grad L at z, the pair and its products in one launch
    void trial_onepass(Iter& it) {
        // 176 VGPRs -> two 256-thread blocks per CU: one resident round of blocks (each block pays the
        // coefficient prologue and a 20-slot reduction epilogue once)
        int gfc = std::min(grid, (env_.gfc > 0 ? env_.gfc : 2) * std::max(1, num_cus));
        // non-temporal loads/stores once the working set (2M + 11 vectors) no longer fits the 256 MB Infinity
        // Cache.  Measured fused-pass times, default policy vs non-temporal: n = 1.25e6 (210 MB) 39.0 / 44.5 us,
        // 1.8e6 (302 MB) 51.0 / 60.4, 2.5e6 (420 MB) 90.1 / 81.5, 5e6 (840 MB) 171 / 159, 1e7 322 / 314.
        // headline family with everything uniform fixed at compile time (see the kernel)
        const int fam = fused_family();
        const bool headline = env_.spec && fam == FAM_HEADLINE;
        const bool spec = headline && it.CV.m == CM;
        // z is the solution the caller reads when the solve stops: once the stop norm is within a factor 10 of
        // the tolerance, store it (one more write stream for the last iteration or two) rather than
        // re-materialise it afterwards with two generic kernels (the same bits either way)
        // ... and during the first 20 iterations of a solve: ALPS subproblems are often that short (13 of them
        // with 180 inner iterations in all on cfg 2), and a stored z costs a tenth of re-materialising one
        // (tol = 0: the caller has said the solve never stops by itself — bench.py's timed region, the step-wise parity
        // tests — so no early stop is being prepared for; whoever asks for z gets it re-materialised, same bits)
        const bool near_stop = (double)stop_norm_ <= 10.0 * opt.tol || (cnt_.k <= 20 && opt.tol > 0.0);
        T* const zstore = (env_.skipz && !near_stop) ? (T*)nullptr : Z_[it.zn].p;
        it.z_skipped = zstore == nullptr;
        const bool small = small_vectors();
        // 0: stored pairs; 2: pairs re-formed from the iterate ring, residuals re-evaluated — possible as soon as every
        // stored pair is a difference of ring neighbours, also with a partial memory (the absent pairs are x - x = 0 with
        // zero coefficients)
        const int m_now = (int)state_.lbfgs.order.size();
        int xr = 0;
        // (the slack form of ALS has its own iterate-history kernel, k_fused_slack_xr: any element-wise kinds)
        if (env_.xr && small && (fam >= 0 || slack) && xr_run_ >= m_now) {
            xr = 2;
            // (only the oldest stored iterate may carry another gamma — see CompactCoef::gam0)
            for (int i = 1; i < m_now; ++i)
                if (gring_[(xc - m_now + i + NXR) % NXR] != (double)state_.gamma) xr = 0;
        }
        if (sy_stale_ && !xr) materialize_pairs();
        if (xr != 2 && !state_.res_valid) ensure_z();
        // the iterate-history form keeps two packs of loads in flight per wave and runs best with ONE wave per
        // SIMD (n = 1e7: 134 vs 140 us; 1.25e6: 28.5 vs 30.2 us): the wave has the vector ALU to itself and
        // the 32-scalar epilogue runs half as often.  (A different grid is a different summation tree: the
        // forms then agree to rounding, not bit for bit — BZ_GFC pins one grid for all of them.)
        // (the slack form's fast instantiations: a full memory, f = DiagQuadratic, no vector-valued parameters of g or D —
        // pipelined like the headline kernel, 256 VGPRs + spill AGPRs: one workgroup per CU there too)
        const bool slack_fast = slack && xr == 2 && env_.slackfast && m_now == CM && desc.f_kind == BZ_F_DIAG_QUADRATIC &&
                                pstreams(false, true, true) == 2 - std::min(2, (int)P.uni) &&
                                !(P.g_u && (P.g_kind == BZ_G_NORM_L1_BOX || P.g_kind == BZ_G_NORM_L0_BOX)) && !P.lambda_vec() && !enet_g;
        // ... with the kinds fixed too (g = NormL1, D = Box: the ALS form of cfg 2), one pack of loads ahead
        const bool slack_hk = slack_fast && env_.slackkind && P.g_kind == BZ_G_NORM_L1 && P.D_kind == BZ_D_BOX;
        if (xr == 2 && env_.gfc <= 0 && (!slack || slack_hk)) gfc = std::min(grid, std::max(1, num_cus));
        for (int k = 0; k < NFC; ++k) slot_n[SL_TRIAL + k] = gfc;
        // (the vectors this pass touches: history + x_d + z + the parameter vectors (+ res, s, y))
        const int nvec = (xr == 2 ? xr2_streams(m_now) : 2 * CM + 5 + pstreams(true, true, true)) + (zstore ? 1 : 0);
        const bool nt = env_.nt >= 0 ? env_.nt != 0 : (double)n * sizeof(T) * nvec > 340e6;
        if (gate_pending_ && xr != 2) gate_abort();
        if (xr == 2 && slack) onepass_slack_xr(it, gfc, zstore, slack_fast, slack_hk);
        else if (xr == 2) onepass_xr2(it, zstore);
        else onepass_stored(it, gfc, zstore, nt, spec, small && spec);
        // (XR = 2 with the gate: the read-back kernel now, so that the next iteration's pass can queue right behind it)
        onepass_scalars(it, xr == 2 && gate_env_);
        if (xr == 2 && gate_env_ && more_coming_ && !opt.verbose && !prof_would_pick(C_FUSED_IT)) gate_prelaunch(it.xd, m_now);
        it.have_trial = true; it.fused_this = true; state_.gx_valid = false; state_.gz_valid = false; it.gram_from_trial = true;
        cnt_.n_grad += 2; cnt_.n_prox += 1;
    }
    // the one-pass trial's scalars: exchanged, folded over the ranks and read back in one launch (p2p, no k_collect), or
    // gathered and, with launch_now, their read-back launched at once (wait_host later)
    void onepass_scalars(Iter& it, bool launch_now) {
        it.tail_used = ctx->p2p_on || launch_now;
        if (ctx->p2p_on) {
            it.tail_ticket = exchange_collect(SL_TRIAL, NFC, 1u << 9);
        } else {
            gather(SL_TRIAL, NFC, 1u << 9);
            if (launch_now) it.tail_ticket = collect_launch_range(SL_TRIAL, NFC, 1u << 9);
        }
    }
    // ALS: the iterate-history pass of the lifted vector (k_fused_slack_xr)
    void onepass_slack_xr(Iter& it, int gfc, T* zstore, bool fast, bool hk) {
        // the m + 1 last iterates of the lifted vector (both halves), the parameter vectors, y ; xs_d (z) out
        const int m_now = (int)state_.lbfgs.order.size();
        SlackIterates<T, CM> SV;
        std::memset(&SV, 0, sizeof(SV));
        SV.m = m_now;
        for (int i = 0; i <= m_now; ++i) SV.XH[i] = X_[(xc - (m_now - i) + NXR) % NXR].p;
        it.CC.gam0 = gring_[(xc - m_now + NXR) % NXR];
        const int slack_streams = 2 * (m_now + 1) + pstreams(true, true, true) + (P.uni >= 2 ? 0 : 1) + 2;      // (pstreams counts D's vector bounds)
        const bool snt = env_.nt >= 0 ? env_.nt != 0 : (double)nx * sizeof(T) * (slack_streams + (zstore ? 2 : 0)) > 340e6;
        mv(slack_streams + (zstore ? 2 : 0), nx);
        form_[C_FUSED_IT] = std::string("k_fused_slack_xr") + (snt ? "<NT=1>" : "<NT=0>");
        // (the fast instantiations: a full memory, f = DiagQuadratic, no vector-valued parameters of g or D)
        if (fast) form_[C_FUSED_IT] += hk ? "(fast,l1-box)" : "(fast)";
        auto go = [&](auto kernel) {
            launch(C_FUSED_IT, kernel, gfc, SV, it.CC, P, (const T*)ymul_.p, state_.gamma, X_[it.xd].p, zstore, nx, parts_.p, (int)SL_TRIAL);
        };
        with_bool(snt, [&](auto nt_) {
            constexpr bool NT = decltype(nt_)::value;
            if (fast) {
                with_uni(P.uni, [&](auto un) {
                    constexpr int UNI = decltype(un)::value;
                    if (hk) go(k_fused_slack_xr<T, CM, NT, true, UNI, 1, 1>);
                    else go(k_fused_slack_xr<T, CM, NT, true, UNI, 0, 0>);
                });
            } else if (m_now == CM) go(k_fused_slack_xr<T, CM, NT, true, -1, 0, 0>);
            else go(k_fused_slack_xr<T, CM, NT, false, -1, 0, 0>);
        });
        sy_stale_ = true; it.res_skipped = true;
        it.trial_ok = false;      // (a tau-backtracked point finishes in the generic chain, after the pairs are re-materialised)
    }
    // the headline or family-table pass on the iterate history (k_fused_compact<XR=2>): released if it was pre-launched
    void onepass_xr2(Iter& it, T* zstore) {
        GatePlan cur;
        if (!xr2_plan(xc, (int)state_.lbfgs.order.size(), gring_, xr_run_, zstore != nullptr, cur))
            throw Error(BZ_ERR_STATE, "the iterate-history pass does not apply");
        it.CC.gam0 = cur.gam0;
        if (gate_pending_ && cur == gate_plan_) {
            // this very launch was made early, behind the previous iteration's read-back: hand it its coefficients
            gate_release(it.CC, zstore);
        } else {
            gate_abort();
            mv(xr2_streams(cur.m_now) + (zstore ? 1 : 0));
            launch_xr2(cur, it.CC, 0, cur.xd, zstore, (T*)nullptr);
        }
        sy_stale_ = true; it.res_skipped = true;
        it.trial_ok = env_.trialfuse != 0; it.trial_plan = cur; it.trial_coef = it.CC;
    }
    // the stored pairs S, Y (k_fused_slack for the lifted vector of ALS, k_fused_compact<XR=0>)
    void onepass_stored(Iter& it, int gfc, T* zstore, bool nt, bool spec, bool off32) {
        if (slack) {
            // the lifted vector [x; s]: res, S[m], Y[m], xs ; xs_d, res, s_new, y_new (z) — both halves — and over n the
            // parameter vectors and the multipliers y
            mv(2 * (2 + 2 * it.CV.m + 4 + (zstore ? 1 : 0)) + pstreams(true, true, true) + (P.uni >= 2 ? 0 : 1), nx);
            form_[C_FUSED] = std::string("k_fused_slack") + (nt ? "<NT=1>" : "<NT=0>");
            with_bool(nt, [&](auto nt_) {
                launch(C_FUSED, k_fused_slack<T, CM, decltype(nt_)::value>, gfc, it.CV, it.CC, (const T*)X_[it.xp].p,
                       (const T*)RES_[it.rp].p, P, (const T*)ymul_.p, state_.gamma, X_[it.xd].p, zstore, RES_[it.rn].p, S_[state_.lbfgs.spare].p,
                       Y_[state_.lbfgs.spare].p, nx, parts_.p, (int)SL_TRIAL);
            });
            return;
        }
        // res, S[m], Y[m], x + the parameter vectors ; x_d, res, s_new, y_new (z)
        mv(2 + 2 * it.CV.m + pstreams(true, true, true) + 4 + (zstore ? 1 : 0));
        form_[C_FUSED] = std::string("k_fused_compact<XR=0") + (spec ? ",SPEC=1" : ",SPEC=0") + (nt ? ",NT=1>" : ",NT=0>");
        auto go = [&](auto kernel) {
            launch(C_FUSED, kernel, gfc, it.CV, it.CC, (const T*)X_[it.xp].p, (const T*)RES_[it.rp].p, P, state_.gamma, X_[it.xd].p,
                   zstore, RES_[it.rn].p, S_[state_.lbfgs.spare].p, Y_[state_.lbfgs.spare].p, n, parts_.p, (int)SL_TRIAL);
        };
        if (off32 && nt) go(k_fused_compact<T, CM, true, true, true>);
        else if (off32) go(k_fused_compact<T, CM, false, true, true>);
        else if (nt && spec) go(k_fused_compact<T, CM, true, true>);
        else if (nt) go(k_fused_compact<T, CM, true, false>);
        else if (spec) go(k_fused_compact<T, CM, false, true>);
        else go(k_fused_compact<T, CM, false, false>);
    }
    // k_fused_sep: the one-pass kernel of the element-wise kinds with the two-loop / Broyden direction
    void trial_sep(Iter& it) {
        if (!state_.res_valid) ensure_z();
        for (int k = 0; k < 12; ++k) slot_n[SL_TRIAL + k] = grid;
        mv((it.tail.mode != 2 ? 2 : 1) + 2 + pstreams(true, true, true) + 5);
        form_[C_FUSED] = "k_fused_sep";
        launch(C_FUSED, k_fused_sep<T>, grid, it.tail, (const T*)X_[it.xp].p, (const T*)RES_[it.rp].p, P, state_.gamma,
               X_[it.xd].p, Z_[it.zn].p, RES_[it.rn].p, S_[state_.lbfgs.spare].p, Y_[state_.lbfgs.spare].p, (T*)nullptr, (T*)nullptr, n,
               parts_.p, (int)SL_TRIAL);
        gather(SL_TRIAL, 12, 1u << 9);
        it.sep_trial = true;
        it.have_trial = true; it.fused_this = true; state_.gx_valid = false; state_.gz_valid = false;
        cnt_.n_grad += 2; cnt_.n_prox += 1;
    }
    // the kernel chain: x_d = x + d (k_dense_head, k_compact_xd or k_axpy_dot), then the stencil passes, or grad L at x_d
    // (affine images or an evaluation); the FB step and the rest follow in finish_chain_trial
    void trial_chain(Iter& it) {
        if (!state_.res_valid) ensure_z();
        // cfg 4 with images: x_d, its images under grad L and c, L(x_d) and the forward-backward step in ONE launch
        // (k_dense_head; single rank, element-wise f, the common prox kinds)
        it.head_on = env_.densesmall && it.use_compact && aff_track_ && !it.stencil_fast_now && !generic_ && !ctx->multi() && !lp_g && !group_g &&
                     !dense_f && state_.gx_valid && state_.gz_valid && state_.aff_count + 1 < aff_refresh_ &&
                     (desc.f_kind == BZ_F_ZERO || desc.f_kind == BZ_F_DIAG_QUADRATIC);
        // x_d = x + d ; gradient at x_d ; state.x = x_d
        const T *res = RES_[it.rp].p, *x = X_[it.xp].p;
        if (it.head_on) {
        } else if (it.use_compact) {
            const CompactVecs<T, CM>& CV = it.CV;
            mv(2 * CV.m + 3);
            // (full memory + a history beyond the Infinity Cache: compile-time trip counts, non-temporal history loads)
            const bool hist_nt = env_.xdnt && (double)n * sizeof(T) * (2 * CV.m + 3) > 340e6;
            // (the template form in the name: a hardware-counter profile is matched to the instantiation that ran)
            nm(CV.m == CM ? (hist_nt ? "k_compact_xd<FULL=1,NT=1>" : "k_compact_xd<FULL=1,NT=0>") : "k_compact_xd<FULL=0,NT=0>");
            if (CV.m == CM && hist_nt) launch(C_XD, k_compact_xd<T, CM, true, true>, grid, CV, it.CC, res, x, X_[it.xd].p, n);
            else if (CV.m == CM) launch(C_XD, k_compact_xd<T, CM, true, false>, grid, CV, it.CC, res, x, X_[it.xd].p, n);
            else launch(C_XD, k_compact_xd<T, CM>, grid, CV, it.CC, res, x, X_[it.xd].p, n);
        } else {
            mv((it.tail.mode != 2 ? 2 : 1) + 2); nm("k_axpy_dot(x_d)");
            launch(C_XD, k_axpy_dot<T>, grid, it.tail, (const T*)nullptr, x, X_[it.xd].p, n, parts_.p, 0);
        }
        if (it.stencil_fast_now) {
            chain_stencil(it);
        } else if (aff_track_) {
            chain_images(it);
        } else {
            algrad(X_[it.xd].p, GX_.p, SL_FXD); ++cnt_.n_grad; state_.gx_valid = true;
        }
    }
    // Stencil5pt: {AL gradient at x_d + FB step} and {AL gradient at z + pair + stop norm} as two passes; same partial
    // sums as the four generic kernels of the first trial
    void chain_stencil(Iter& it) {
        const int xd = it.xd, zn = it.zn;
        for (int sidx = SL_FXD; sidx <= SL_STOP; ++sidx) slot_n[sidx] = grid;
        // (uniform penalties / zero multipliers travel as numbers, P.uni: the two stencil passes stream mu and mu*y
        // otherwise — 4 of the iteration's 43 passes)
        // (r03: with the compact form the second pass re-forms res from x_d and z — k_stencil_update_c<REGX = 1> — instead of
        // reading it)
        const int regx = it.use_compact && env_.stencil_regx > 0 ? 1 : 0;
        mv(2 + pstreams(false, true, true) + 3);        // x_d, b + parameters ; grad, z, res
        const StencilHalo<T> halo_x = halo_exchange(X_[xd].p);
        const bool fb_nt = env_.xdnt && (double)n * sizeof(T) * 12 > 340e6;
        nm(fb_nt ? "k_stencil_fb<NT=1>" : "k_stencil_fb<NT=0>");
        with_bool(fb_nt, [&](auto nt_) {
            launch(C_STENCIL_FB, k_stencil_fb<T, decltype(nt_)::value>, grid, (const T*)X_[xd].p, P, (int64_t)desc.f_grid_nx,
                   (int64_t)desc.f_grid_ny, state_.gamma, GX_.p, Z_[zn].p, RES_[it.rn].p, n, parts_.p,
                   (int)SL_FXD, (int)SL_GSUM, halo_x);
        });
        const StencilHalo<T> halo_z = halo_exchange(Z_[zn].p);
        if (it.use_compact) {
            // ... with the Gram products of the new pair and the next application's p, w in the same pass
            // (r03: this pass — 19 streams, 27 accumulators — runs best with ONE workgroup per CU, one resident round and a
            // 27-slot epilogue per CU: 102 us against 108 with two or four and 114 on the problem's grid of 2048, at 2048^2 ;
            // the other two passes want the largest grid.  BZ_SUC_GRID=k: k per CU, 0: `grid`.)
            const CompactVecs<T, CM>& CV = it.CV;
            const int g_upd = env_.suc_grid > 0 ? std::min(grid, env_.suc_grid * std::max(1, num_cus)) : grid;
            for (int sidx = 0; sidx < NFC; ++sidx) slot_n[SL_TRIAL + sidx] = sidx < 5 ? grid : g_upd;      // (slots 0..4: k_stencil_fb's)
            mv(2 + pstreams(false, true, false) + (5 - regx) + 2 + 2 * CV.m);
            const bool hist_nt = env_.xdnt && (double)n * sizeof(T) * (2 * CV.m + 12) > 340e6;
            static const char* const forms[2][3] = {
                {"k_stencil_update_c<FULL=0,NT=0>", "k_stencil_update_c<FULL=1,NT=0>", "k_stencil_update_c<FULL=1,NT=1>"},
                {"k_stencil_update_c<FULL=0,NT=0,REGX=1>", "k_stencil_update_c<FULL=1,NT=0,REGX=1>", "k_stencil_update_c<FULL=1,NT=1,REGX=1>"}};
            nm(forms[regx][CV.m == CM ? 1 + hist_nt : 0]);
            auto go = [&](auto full_, auto nt_) {
                constexpr bool FULL = decltype(full_)::value, NT = decltype(nt_)::value;
                auto run = [&](auto kernel) {
                    launch(C_STENCIL_UPD, kernel, g_upd, CV, (const T*)Z_[zn].p, P, (int64_t)desc.f_grid_nx, (int64_t)desc.f_grid_ny,
                           (const T*)X_[xd].p, (const T*)X_[it.xp].p, (const T*)RES_[it.rn].p, (const T*)RES_[it.rp].p,
                           (const T*)GX_.p, state_.gamma, S_[state_.lbfgs.spare].p, Y_[state_.lbfgs.spare].p, n, parts_.p, (int)SL_TRIAL, halo_z);
                };
                if (regx == 1) run(k_stencil_update_c<T, CM, FULL, NT, 1>);
                else run(k_stencil_update_c<T, CM, FULL, NT, 0>);
            };
            if (CV.m == CM && hist_nt) go(std::true_type{}, std::true_type{});
            else if (CV.m == CM) go(std::true_type{}, std::false_type{});
            else go(std::false_type{}, std::false_type{});
            if (ctx->p2p_on) {
                // exchange + fold over the ranks + read-back of all 32 slots in one launch
                it.tail_ticket = exchange_collect(SL_TRIAL, NFC, 1u << 9);
                it.tail_used = true;
            }
            it.gram_from_trial = true;
        } else {
            mv(2 + pstreams(false, true, false) + 5 + 2);   // z, b + parameters, x_d, x, res, res_prev, grad ; s, y
            nm("k_stencil_update");
            launch(C_STENCIL_UPD, k_stencil_update<T>, grid, (const T*)Z_[zn].p, P, (int64_t)desc.f_grid_nx,
                   (int64_t)desc.f_grid_ny, (const T*)X_[xd].p, (const T*)X_[it.xp].p, (const T*)RES_[it.rn].p,
                   (const T*)RES_[it.rp].p, (const T*)GX_.p, state_.gamma, S_[state_.lbfgs.spare].p, Y_[state_.lbfgs.spare].p, (T*)nullptr, n, parts_.p,
                   (int)SL_FZ, (int)SL_YS, halo_z);
        }
        it.have_trial = true; state_.gx_valid = true; state_.gz_valid = false;
        cnt_.n_grad += 2; cnt_.n_prox += 1;
    }
    // cfg 4: gradient (and c) at x_d into the candidate buffers — the same combination of the held images that forms x_d
    // (k_dense_head, or k_affine_image and the value L(x_d)), or an evaluation — then trade: GX_ = grad L(x_d),
    // GXN_ = grad L(x_prev)
    void chain_images(Iter& it) {
        it.state_imgs = state_.gx_valid && state_.gz_valid;      // (the images of this state's x and z are what GX_, GZ_, CXS_, CZS_ hold)
        if (it.use_compact && state_.gx_valid && state_.gz_valid && state_.aff_count + 1 < aff_refresh_) {
            ++state_.aff_count; ++state_.n_affine; it.img_trial = true;
            CompactVecs<T, CM> VA = image_vecs(true), VG = image_vecs(false);
            if (it.head_on) {
                DenseHeadArgs<T, CM> a;
                std::memset(&a, 0, sizeof(a));
                a.V = it.CV; a.VG = VG; a.VA = VA; a.C = it.CC;
                a.res = RES_[it.rp].p; a.x = X_[it.xp].p; a.x_d = X_[it.xd].p;
                a.gbase = GX_.p; a.gzimg = GZ_.p; a.gout = GXN_.p;
                a.cbase = CXS_.p; a.czimg = CZS_.p; a.cout = CXD_.p; a.yupd = YU_.p;
                a.z = Z_[it.zn].p; a.res_new = RES_[it.rn].p; a.gamma = state_.gamma;
                a.n = n; a.ny = ny; a.parts = parts_.p;
                a.slot_f = SL_FXD; a.slot_pen = SL_PXD; a.slot_fb = SL_GSUM; a.gn = grid; a.gy = grid_y;
                slot_n[SL_FXD] = grid; slot_n[SL_PXD] = grid_y;
                for (int kk = 0; kk < 3; ++kk) slot_n[SL_GSUM + kk] = grid;
                // (what the six kernels move: k_compact_xd, the two images, f, yupd, the FB step)
                mv(2 * it.CV.m + 3); mv(2 * VA.m + 3, ny); mv(2 * VG.m + 3); mv(1 + pstreams(true, false, false));
                mv(2 + pstreams(false, true, false), ny); mv(4 + pstreams(false, false, true));
                nm("k_dense_head");
                launch(C_MISC, k_dense_head<T, CM>, grid + grid_y, a, P);
                it.head_fb = true;
            } else {
                mv(2 * VA.m + 3, ny); nm("k_affine_image");
                launch(C_MISC, k_affine_image<T, CM>, grid_y, VA, it.CC, (const T*)CXS_.p, (const T*)CZS_.p, CXD_.p, ny);
                mv(2 * VG.m + 3);
                launch(C_MISC, k_affine_image<T, CM>, grid, VG, it.CC, (const T*)GX_.p, (const T*)GZ_.p, GXN_.p, n);
                // the value L(x_d): f element-wise, the penalty from the image of c
                slot_n[SL_FXD] = grid; slot_n[SL_PXD] = grid_y;
                mv(1 + pstreams(true, false, false));
                launch(C_MISC, k_fvalue_elem<T>, grid, (const T*)X_[it.xd].p, P, n, parts_.p, (int)SL_FXD, (const T*)nullptr);
                mv(2 + pstreams(false, true, false), ny);
                launch(C_MISC, k_yupd<T>, grid_y, (const T*)CXD_.p, P, YU_.p, ny, parts_.p, (int)SL_PXD);
            }
        } else {
            state_.aff_count = 0;
            cx_keep_ = CXD_.p;
            algrad(X_[it.xd].p, GXN_.p, SL_FXD);
            cx_keep_ = nullptr;
        }
        GX_.swap(GXN_);
        ++cnt_.n_grad; state_.gx_valid = true;
    }

    // a trial of the kernel chain from grad L at the trial point on: the FB step, grad L at z, then k_dense_tail, or
    // k_update_c / k_update and the pair's images
    void finish_chain_trial(Iter& it) {
        const int zn = it.zn, rn = it.rn, xcur = it.xcur;
        if (!state_.gx_valid) { algrad(X_[xcur].p, GX_.p, SL_FXD); state_.gx_valid = true; }
        if (it.head_fb) it.head_fb = false;      // (k_dense_head made this step already)
        else fbstep(X_[xcur].p, GX_.p, state_.gamma, Z_[zn].p, RES_[rn].p, SL_GSUM);
        gather(SL_GSUM, 3, 0u);
        ++cnt_.n_prox;
        T* const gz_dst = aff_track_ ? GZN_.p : GZ_.p;      // (affine images: grad L(z_prev) is still needed)
        if (aff_track_) cx_keep_ = CZN_.p;
        // cfg 4: the fold of the row-group partials, the pair with its products and the pair's images in ONE launch
        // behind the pass over A (k_dense_tail)
        const bool tail_on = env_.densesmall && aff_track_ && compact_ok && !generic_ && !ctx->multi() &&
                             desc.c_kind == BZ_C_DENSE_AFFINE && dense_fused_on();
        if (tail_on) {
            slot_n[SL_FZ] = grid;
            dense_fused_launch(Z_[zn].p, SL_FZ + 1);
            ++cnt_.n_grad; state_.gz_valid = true;
            cx_keep_ = nullptr;
            const CompactVecs<T, CM> VG = compact_vecs();
            DenseTailArgs<T, CM> a;
            std::memset(&a, 0, sizeof(a));
            a.V = VG; a.part = GT_.p; a.nchunks = df_groups_; a.pstride = npad;
            a.z = Z_[zn].p; a.gz = gz_dst;
            a.x = X_[xcur].p; a.x_prev = X_[it.xp].p; a.res = RES_[rn].p; a.res_prev = RES_[it.rp].p; a.gx = GX_.p;
            a.gamma = state_.gamma; a.s_new = S_[state_.lbfgs.spare].p; a.y_new = Y_[state_.lbfgs.spare].p;
            a.gx_prev = GXN_.p; a.gz_prev = GZ_.p; a.gs_img = GS_[state_.lbfgs.spare].p; a.gy_img = GY_[state_.lbfgs.spare].p;
            a.cx = CXD_.p; a.cx_prev = CXS_.p; a.cz = CZN_.p; a.cz_prev = CZS_.p;
            a.cs_img = AS_[state_.lbfgs.spare].p; a.cy_img = AY_[state_.lbfgs.spare].p;
            a.n = n; a.ny = ny; a.parts = parts_.p; a.slot_fz = SL_FZ; a.slot_upd = SL_YS; a.gn = grid; a.gy = grid_y;
            for (int kk = 0; kk < 3 + 4 * CM + 2; ++kk) slot_n[SL_YS + kk] = grid;
            // (what the four kernels move: the fold + f terms, k_update_c, the two image pairs)
            mv(df_groups_ + 2 + pstreams(true, false, false)); mv(8 + 2 * VG.m); mv(6, ny); mv(6);
            nm("k_dense_tail");
            launch(C_UPDATE, k_dense_tail<T, CM>, grid + grid_y, a, P);
            gather(SL_FZ, 2, 0u, 2u);
            gather(SL_YS, 3 + 4 * CM + 2, 4u);
            it.gen_gram = true; it.m_gram = VG.m; it.tail_used = false;
            return;
        }
        algrad(Z_[zn].p, gz_dst, SL_FZ); ++cnt_.n_grad; state_.gz_valid = true;
        cx_keep_ = nullptr;
        if (compact_ok) {
            // the pair, the stop norm AND the compact form's products (Gram products of the candidate pair, the
            // next application's p, w) in one pass and one read-back — against the memory as it is NOW
            const CompactVecs<T, CM> VG = compact_vecs();
            for (int kk = 0; kk < 3 + 4 * CM + 2; ++kk) slot_n[SL_YS + kk] = grid;
            mv(8 + 2 * VG.m); nm("k_update_c");
            launch(C_UPDATE, k_update_c<T, CM>, grid, VG, (const T*)X_[xcur].p, (const T*)X_[it.xp].p,
                   (const T*)RES_[rn].p, (const T*)RES_[it.rp].p, (const T*)GX_.p, (const T*)gz_dst, state_.gamma,
                   S_[state_.lbfgs.spare].p, Y_[state_.lbfgs.spare].p, n, parts_.p, (int)SL_TRIAL);
            gather(SL_YS, 3 + 4 * CM + 2, 4u);
            it.gen_gram = true; it.m_gram = VG.m; it.tail_used = false;
        } else {
            for (int kk = 0; kk < 3; ++kk) slot_n[SL_YS + kk] = grid;
            mv(8);
            launch(C_UPDATE, k_update<T>, grid, (const T*)X_[xcur].p, (const T*)X_[it.xp].p,
                   (const T*)RES_[rn].p, (const T*)RES_[it.rp].p, (const T*)GX_.p, (const T*)gz_dst, state_.gamma,
                   S_[state_.lbfgs.spare].p, Y_[state_.lbfgs.spare].p, n, parts_.p, (int)SL_YS);
            gather(SL_YS, 3, 4u);
        }
        if (aff_track_) {
            // images of the candidate pair (s = x - x_prev, y = res - res_prev) under c and grad L
            mv(6, ny);
            launch(C_MISC, k_image_pair<T>, grid_y, (const T*)CXD_.p, (const T*)CXS_.p, (const T*)CZN_.p,
                   (const T*)CZS_.p, AS_[state_.lbfgs.spare].p, AY_[state_.lbfgs.spare].p, ny);
            mv(6);
            launch(C_MISC, k_image_pair<T>, grid, (const T*)GX_.p, (const T*)GXN_.p, (const T*)GZN_.p,
                   (const T*)GZ_.p, GS_[state_.lbfgs.spare].p, GY_[state_.lbfgs.spare].p, n);
        }
    }

    // the step-size test on the trial's scalars: gamma halvings (a failing test on images is re-run on evaluations
    // first), tau backtracks
    void step_size_test(Iter& it) {
        const T eps = std::numeric_limits<T>::epsilon();
        const int max_bt = opt.max_backtracks;
        T sigma = beta * (T(0.5) / state_.gamma) * (T(1) - alpha);
        const T tol0 = T(10) * eps * (T(1) + std::abs(it.FBE_x));
        const T threshold = it.FBE_x - sigma * (it.nr0 * it.nr0) + tol0;
        std::vector<double>& v = it.v;
        for (int k = 1; k <= max_bt; ++k) {
            if (!it.have_trial) finish_chain_trial(it);
            if ((it.have_trial && it.gram_from_trial) || it.gen_gram) {
                v = (it.have_trial && it.tail_used) ? wait_host(NFC, it.tail_ticket) : collect_range(SL_TRIAL, NFC, 1u << 9);
                it.gram_from_trial = true; it.gen_gram = false;
                for (int i = 0; i < CM; ++i) {
                    it.gsy[i] = v[10 + i]; it.gyy[i] = v[10 + CM + i];
                    it.tp[i] = v[10 + 2 * CM + i]; it.tw[i] = v[10 + 3 * CM + i];
                }
                it.tpn = v[10 + 4 * CM]; it.twn = v[10 + 4 * CM + 1];
            } else if (it.have_trial && it.sep_trial) {
                static_assert(SL_TRIAL == SL_FXD && SL_STOP == SL_TRIAL + 9 && SL_GU == SL_TRIAL + 10, "k_fused_sep's slots");
                v = collect_range(SL_TRIAL, 12, 1u << 9);
                it.sep_p = v[10]; it.sep_w = v[11];
                it.gram_from_trial = false;
            } else {
                v = collect({SL_FXD, SL_PXD, SL_GSUM, SL_DOT, SL_SS, SL_FZ, SL_PZ, SL_YS, SL_YTY, SL_STOP},
                            1u << 9);
                it.gram_from_trial = false;
            }
            it.have_trial = false;
            state_.f_x = al_value(v[0], v[1]);
            state_.g_z = g_value(v[2]); state_.dot_gr = T(v[3]); state_.ss_res = T(v[4]);
            const T f_z = al_value(v[5], v[6]);
            state_.fraw_last = f_value(v[5]); state_.f_z_al = f_z;
            const T nr = std::sqrt(state_.ss_res);
            const T f_z_upp = state_.f_x - state_.dot_gr + ((alpha / state_.gamma) / T(2)) * (nr * nr);
            const T tol = T(10) * eps * (T(1) + std::abs(f_z));
            const bool halve = adaptive_ && std::isfinite((double)state_.gamma) && f_z > f_z_upp + tol && state_.gamma >= min_gamma;
            if (halve && it.img_trial) {
                // The step-size test compares f(z) with a model built on f(x) and grad L(x) to within 10 eps: an image
                // (a linear combination, not an evaluation) is not consistent with f(z) to that level near convergence,
                // and a value a few ulps low would halve gamma again and again at the same point.  A FAILING test is
                // therefore never trusted on images: evaluate f and grad L at this x with the two passes over A and
                // run the trial again (this does not consume one of the max_backtracks trials).
                it.img_trial = false; state_.aff_count = 0; ++state_.n_affine_verify;
                cx_keep_ = CXD_.p;
                algrad(X_[it.xcur].p, GX_.p, SL_FXD); ++cnt_.n_grad; state_.gx_valid = true;
                cx_keep_ = nullptr;
                --k;
                continue;
            }
            const T FBE_new = f_z_upp + state_.g_z;
            // not a plain iteration: z of the state this step started from may be needed (z_curr below), and
            // it must be formed with the gamma of that state
            // ... and the classic kernels that finish this iteration need the stored pairs (and the residual of
            // that state) as vectors
            // a pass pre-launched for the next iteration assumed this trial is accepted and its pair inserted
            if (gate_pending_ && !(k == 1 && !halve && (FBE_new <= threshold || k >= max_bt) && T(v[7]) > T(0))) gate_abort();
            it.halved_last = halve && k >= max_bt;
            if (it.halved_last) { it.last_fused = it.fused_this; it.last_ring = sy_stale_; it.gamma_res = state_.gamma; }
            if (halve) it.trial_ok = false;
            if (sy_stale_ && !it.trial_ok && (halve || !(FBE_new <= threshold || k >= max_bt))) materialize_pairs();
            if ((!state_.z_valid || !state_.res_valid) && (halve || !(FBE_new <= threshold || k >= max_bt))) ensure_z();
            if (halve) {
                it.halved_here = true;
                state_.gamma = state_.gamma * T(0.5); ++cnt_.n_halv;
                if (state_.gamma < min_gamma)
                    std::fprintf(stderr, "Warning: stepsize `gamma` became too small (%g)\n", (double)state_.gamma);
                sigma = sigma * T(2);   // (as upstream: sigma is updated, the threshold is kept)
                lbfgs_reset();
                it.fused_this = false; it.reset_this = true;
                continue;
            }
            if (FBE_new <= threshold || k >= max_bt) break;
            tau = (k >= max_bt - 1) ? T(0) : tau / T(2);
            ++it.nbt; ++cnt_.n_bt;
            retrial(it);
        }
    }
    // the tau-backtracked point x_d tau + z (1 - tau) into the blend buffer, and its trial: through the one-pass kernel
    // (trial given), on the blended images (cfg 4), or with an evaluation of grad L
    void retrial(Iter& it) {
        const int xb = it.xb;
        mv(3);
        launch(C_MISC, k_blend<T>, grid, (const T*)X_[it.xd].p, (const T*)Z_[it.zp].p, tau, T(1) - tau, X_[xb].p, n);
        it.xcur = xb;
        it.fused_this = false;
        if (it.trial_ok) {
            // the blended point through the one-pass kernel: given in X_[xb], evaluated against the same ring
            // of iterates; z and res of the new state are stored (Z_[zn], RES_[rn])
            for (int kk = 0; kk < NFC; ++kk) slot_n[SL_TRIAL + kk] = it.trial_plan.gfc;
            // the iterates, the parameter vectors (mu, mu*y unless numbers), the trial point ; z, res
            mv(xr2_streams(it.m_at_trial) + 2);
            launch_xr2(it.trial_plan, it.trial_coef, 1, X_[xb].p, Z_[it.zn].p, RES_[it.rn].p);
            onepass_scalars(it, false);
            it.have_trial = true; it.gram_from_trial = true; state_.gx_valid = false; state_.gz_valid = false;
            cnt_.n_grad += 2; cnt_.n_prox += 1;
        } else if (env_.affine_blend && aff_track_ && it.state_imgs && state_.gx_valid && it.nbt == 1 && !it.halved_here && compact_ok &&
                   !generic_ && !ctx->multi() && state_.aff_count + 1 < aff_refresh_) {
            // cfg 4, first tau backtrack of an iteration: the blended point is an affine combination of x_d and the state's z,
            // whose images under c and grad L are at hand — its images are the same combination (k_blend's operations), no
            // pass over A.  (As for x_d: a failing step-size test on images is re-run on evaluations, img_trial.)  The rejected
            // trial's z images (CZN_, GZN_) are dead: they take the results and trade places.
            ++state_.aff_count; it.img_trial = true;      // (n_affine_images counts iterations whose trial point x + d went on images)
            ++state_.n_affine_blends;
            mv(3, ny);
            launch(C_MISC, k_blend<T>, grid_y, (const T*)CXD_.p, (const T*)CZS_.p, tau, T(1) - tau, CZN_.p, ny);
            CXD_.swap(CZN_);
            mv(3);
            launch(C_MISC, k_blend<T>, grid, (const T*)GX_.p, (const T*)GZ_.p, tau, T(1) - tau, GZN_.p, n);
            GX_.swap(GZN_);
            slot_n[SL_FXD] = grid; slot_n[SL_PXD] = grid_y;
            mv(1 + pstreams(true, false, false));
            launch(C_MISC, k_fvalue_elem<T>, grid, (const T*)X_[xb].p, P, n, parts_.p, (int)SL_FXD, (const T*)nullptr);
            mv(2 + pstreams(false, true, false), ny);
            launch(C_MISC, k_yupd<T>, grid_y, (const T*)CXD_.p, P, YU_.p, ny, parts_.p, (int)SL_PXD);
            ++cnt_.n_grad; state_.gx_valid = true;
        } else {
            if (aff_track_) { cx_keep_ = CXD_.p; state_.aff_count = 0; it.img_trial = false; }
            algrad(X_[xb].p, GX_.p, SL_FXD); ++cnt_.n_grad; state_.gx_valid = true;
            cx_keep_ = nullptr;
        }
    }

    // the accepted trial becomes the state: image trade, pair insertion (or k_gram_pair), the x_b swap, the ring counters
    // and the validity flags
    void commit(Iter& it) {
        if (aff_track_) {
            // the accepted state's images become the current ones
            GZ_.swap(GZN_);
            CZS_.swap(CZN_);
            CXS_.swap(CXD_);
        }
        // update!(H, x - x_prev, res - res_prev): the pair sits in the spare slot
        const T ys = T(it.v[7]), yty = T(it.v[8]);
        last_ys = ys;
        // p, w for the next application: valid iff the accepted point is the one the fused trial measured
        // and the memory was not reset meanwhile (gram_insert shifts them along with the Gram matrices)
        state_.lbfgs.pw_valid = compact_ok && it.gram_from_trial && (int)state_.lbfgs.order.size() == it.m_gram;
        if (state_.lbfgs.pw_valid) {
            for (int i = 0; i < CM; ++i) { state_.lbfgs.hp[i] = i < it.m_gram ? it.tp[i] : 0.0; state_.lbfgs.hw[i] = i < it.m_gram ? it.tw[i] : 0.0; }
            state_.lbfgs.p_new = it.tpn; state_.lbfgs.w_new = it.twn;
        } else if (compact_ok && it.sep_trial && it.fused_this && it.m_at_trial == 0 && state_.lbfgs.order.empty()) {
            // first iteration of a solve (empty memory): the k_fused_sep pass measured the new pair's p and w
            state_.lbfgs.pw_valid = true;
            for (int i = 0; i < CM; ++i) { state_.lbfgs.hp[i] = 0.0; state_.lbfgs.hw[i] = 0.0; }
            state_.lbfgs.p_new = it.sep_p; state_.lbfgs.w_new = it.sep_w;
        }
        if (dir_kind_ == BZ_DIR_BROYDEN) {
            broyden_update();                    // (no curvature test: every pair updates the operator)
        } else if (ys > T(0) || dir_kind_ == BZ_DIR_ANDERSON) {
            if (compact_ok && !it.gram_from_trial && !state_.lbfgs.order.empty()) {
                // the accepted pair is not the one the fused trial measured: its Gram products with the
                // stored pairs come from their own pass
                for (int k = 0; k < 2 * CM; ++k) slot_n[SL_GU + k] = grid;
                mv(2 * (int)state_.lbfgs.order.size() + 1);
                launch(C_DOT, k_gram_pair<T, CM>, grid, compact_vecs(), (const T*)Y_[state_.lbfgs.spare].p, n, parts_.p,
                       (int)SL_GU);
                gather(SL_GU, 2 * CM, 0u);
                auto gv = collect_range(SL_GU, 2 * CM, 0u);
                for (int i = 0; i < CM; ++i) { it.gsy[i] = gv[i]; it.gyy[i] = gv[CM + i]; }
            }
            state_.lbfgs.insert(ys, yty, it.gsy, it.gyy, compact_ok, dir_kind_ == BZ_DIR_ANDERSON);
        } else {
            ++cnt_.n_skips;
            materialize_pairs();         // (history as iterates: the window stops being contiguous here)
        }
        // A tau-backtracked point sits in the blend buffer: trade the two buffers so that the accepted iterate is
        // the next one of the ring whatever produced it — the stored pairs stay the successive differences of
        // the ring's last iterates, and the run below goes on through backtracks
        if (it.xcur == it.xb && fused_ok && compact_ok) {
            X_[it.xd].swap(X_[it.xb]);
            it.xcur = it.xd;
        }
        // history as iterates is possible after CM iterations in a row that each inserted their pair, with no
        // change of gamma (which resets the memory) in between
        // (xr_run_: how many of the newest stored pairs are differences of ring neighbours.  The pair of an
        // iteration that halved gamma is one too — y = res_new(gamma/2) - res_prev(gamma), as upstream has it —
        // because every iterate in the ring remembers the gamma of its residual, gring_)
        const bool inserted = ys > T(0) || dir_kind_ == BZ_DIR_ANDERSON;
        xr_run_ = (fused_ok && compact_ok && inserted && it.xcur == it.xd) ? (it.reset_this ? 1 : xr_run_ + 1) : 0;
        gring_[it.xcur] = (double)state_.gamma;
        stop_norm_ = it.v[9];
        xc = it.xcur; rc = it.rn; zc = it.zn;
        // the generic trial writes z; an accepted fused one may not have, nor res.  (The trial that became the state: the
        // accepted one, or the last one where the loop ended on its halving, fused_this being cleared by then)
        const bool trial_fused = it.halved_last ? it.last_fused : it.fused_this;
        state_.z_valid = !(it.z_skipped && trial_fused);
        state_.res_valid = !(it.res_skipped && trial_fused);
        if (it.halved_last) {
            // The loop ended on a halving in its last trial.  That trial was not repeated: it is the new state, and its z,
            // res and pair belong to the gamma before the halving, as upstream has it.  The iterate-history passes would
            // re-evaluate this iterate's residual with the halved gamma, so the run of ring differences starts over and
            // the ring remembers the gamma the residual was formed with.  What the trial did not leave as vectors (a
            // one-pass launch stores neither res nor, as a rule, z; the iterate-history forms keep the pair in the ring)
            // is formed here, with that gamma.
            xr_run_ = 0;
            gring_[xc] = (double)it.gamma_res;
            if (it.last_ring && inserted && it.xcur == it.xd) { sy_stale_ = true; materialize_pairs(gring_[xc]); }
            ensure_z(true, it.gamma_res);
        }
        last_nbt = it.nbt; last_fused = it.fused_this;
        if (it.fused_this) ++cnt_.n_fused;
    }
   private:
    void fill_stats(bz_panoc_stats* st) {
        std::memset(st, 0, sizeof(*st));
        st->iters = cnt_.k; st->f_z = (double)state_.fraw_last; st->g_z = (double)state_.g_z; st->al_z = (double)state_.f_z_al;
        st->gamma = (double)state_.gamma; st->tau = (double)tau; st->stop_norm = stop_norm_;
        st->n_grad = cnt_.n_grad; st->n_prox = cnt_.n_prox; st->n_backtracks = cnt_.n_bt; st->n_gamma_halvings = cnt_.n_halv;
        st->n_fused_iters = cnt_.n_fused; st->n_lbfgs_skips = cnt_.n_skips;
        st->elapsed_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        st->status = std::isnan((double)state_.f_x) ? 2 : ((double)stop_norm_ <= opt.tol ? 0 : 1);
        st->persist_fallbacks = (int32_t)n_persist_fallbacks_;
        st->n_affine_images = state_.n_affine;
        st->n_gated_launches = n_gated_;
        st->n_gate_aborts = n_gate_aborts_;
        st->n_gate_fallbacks = n_gate_fallbacks_;
        st->n_dense_onepass = n_dense_onepass_;
        st->n_dense_fallbacks = n_dense_fallbacks_;
        st->n_affine_blends = state_.n_affine_blends;
    }

    // ---- a row-wise sparse f (kept behind every older member: their layout is the parent's).  SparseLeastSquares,
    // SparseLogistic, SparseGLM, SparseMultinomial and SparseMultiGLM are one path, `sparse_ls`: a pass over A_f that leaves r and the rows'
    // losses, then the passes over A_f' on r.  What a kind differs in is one row, copied to spf_ at creation:
    struct SparseRowF {
        int f_kind;
        const char *name, *noun, *b;       // in the messages: the kind, "a sparse <noun> f" and what the kind calls its vector
        int mode;                          // the epilogue of the pass over A_f (from SPMM_SOFTMAX on: the K-wide kernels of bz_spmm.h)
        bool weighted;                     // the epilogue takes w, w_uniform and delta (one more stream with a weight vector)
    };
    static constexpr SparseRowF SPARSE_ROW_F[] = {
        {BZ_F_SPARSE_LEAST_SQUARES, "SparseLeastSquares", "least-squares", "b[m]", SP_LS_R, false},
        {BZ_F_SPARSE_LOGISTIC, "SparseLogistic", "logistic", "the labels b[m]", SP_LOGIT_R, false},
        {BZ_F_SPARSE_GLM, "SparseGLM", "GLM", "b[m]", SP_GLM_MODE0, true},       // (mode and weighted: from f_loss, f_w and f_scale)
        {BZ_F_SPARSE_MULTINOMIAL, "SparseMultinomial", "multinomial", "the labels b[m]", SPMM_SOFTMAX, true},
        {BZ_F_SPARSE_MULTI_GLM, "SparseMultiGLM", "multi-response GLM", "B[m][K]", SPMM_GLM_MODE0, true},      // (mode: from f_loss)
    };
    SparseRowF spf_ = SPARSE_ROW_F[0];
    bool sparse_ls = false, sparse_mn = false;     // (sparse_mn: spf_.mode == SPMM_SOFTMAX, the softmax and its label check)
    bool sparse_kw = false;                // the K-wide kernels of bz_spmm.h: the multinomial and the multi-response GLM f
    SpCsr spF_, spFt_;                     // A_f (m x n) and A_f' (n x m)
    DBuf<T> glm_w_;                        // [m] scale * w, or empty: glm_w_uniform_ = scale for every row
    T glm_w_uniform_ = T(1), glm_delta_ = T(0);
    int mn_K_ = 0, mn_KP_ = 0;             // the K-wide kinds: the classes / responses, and the power of two >= K
};

// one-pass kernel of an oracle family: the instantiations live in bz_families_dk*.hip (one file per D class, so that
// they compile in parallel)
template <class T> FusedFn<T> family_kernel(int fam, bool nt, int uni) {
    switch (fam_dk(fam)) {
    case FAM_D_ZERO: return family_kernel_dk<T, FAM_D_ZERO>(fam, nt, uni);
    case FAM_D_FREE: return family_kernel_dk<T, FAM_D_FREE>(fam, nt, uni);
    case FAM_D_BOX: return family_kernel_dk<T, FAM_D_BOX>(fam, nt, uni);
    case FAM_D_BOX_VEC: return family_kernel_dk<T, FAM_D_BOX_VEC>(fam, nt, uni);
    case FAM_D_VC: return family_kernel_dk<T, FAM_D_VC>(fam, nt, uni);
    case FAM_D_CC: return family_kernel_dk<T, FAM_D_CC>(fam, nt, uni);
    case FAM_D_EITHEROR: return family_kernel_dk<T, FAM_D_EITHEROR>(fam, nt, uni);
    case FAM_D_XOR: return family_kernel_dk<T, FAM_D_XOR>(fam, nt, uni);
    default: return nullptr;
    }
}

SolverBase* make_solver(Ctx* ctx, const bz_problem_desc& d) {
    if (d.dtype == BZ_F64) return new Solver<double>(ctx, d);
    if (d.dtype == BZ_F32) return new Solver<float>(ctx, d);
    throw Error(BZ_ERR_ARG, "dtype must be BZ_F64 or BZ_F32");
}

}  // namespace bz
