// Adversarial objectives on the discriminators' LOGITS (trainer.py --gan_loss; include/discogan_hip.h): per problem
//   loss = mean_i f(x_i),   dlogit_i = gout f'(x_i) / n
// with the target tau by role (D_REAL: real_label, D_FAKE: 0, G_FAKE: 1) and
//   BCE on logits   f = tau sp(-x) + (1 - tau) sp(x)   f' = sigmoid(x) - tau      sp(x) = max(x, 0) + log1p(exp(-|x|))
//   LSGAN           f = (x - tau)^2                    f' = 2 (x - tau)           (no 1/2: CycleGAN's form)
//   hinge           D_REAL max(0, 1 - x) | D_FAKE max(0, 1 + x) | G_FAKE -x       f' = -[x < 1] | +[x > -1] | -1, 0 at the kink
// Everything of sp and sigmoid comes from e = exp(-|x|), so a saturated logit keeps a relatively accurate, non-zero gradient
// (tau = 1: -sigmoid(-x), tau = 0: sigmoid(x); never log(sigmoid(x)), never 1 - sigmoid(x)).  kind, role and tau are the same for a
// whole problem: the branches on them are uniform.  A NaN logit gives a NaN term and a NaN derivative in every kind and role (the
// hinge is written with comparisons that fall through to x for a NaN).  Forward: one 256-thread workgroup per problem, partial sums in
// double, reduced in bce_fwd_kernel's fixed order -- no atomics, no workspace, a repeat is bitwise the same.
#include "dg_common.h"
#include <math.h>

struct DgGanRoles {
    int v[DG_MAX_GROUPS];
};

__device__ __forceinline__ float gan_tau(int role, float real_label) {
    return role == DG_GAN_D_REAL ? real_label : (role == DG_GAN_G_FAKE ? 1.f : 0.f);
}

__device__ __forceinline__ float gan_term(int kind, int role, float tau, float x) {
    if (kind == DG_GAN_LSGAN) {
        const float d = x - tau;
        return d * d;
    }
    if (kind == DG_GAN_HINGE) {
        if (role == DG_GAN_G_FAKE) return -x;
        const float t = role == DG_GAN_D_REAL ? 1.f - x : 1.f + x;
        return t <= 0.f ? 0.f : t;                                          // a NaN fails the comparison and stays
    }
    // tau sp(-x) + (1 - tau) sp(x): both softplus share log1p(e), and tau + (1 - tau) is exactly 1
    const float l = log1pf(expf(-fabsf(x)));
    return l + (x > 0.f ? (1.f - tau) * x : -tau * x);
}

__device__ __forceinline__ float gan_deriv(int kind, int role, float tau, float x) {
    if (kind == DG_GAN_LSGAN) return 2.f * (x - tau);
    if (kind == DG_GAN_HINGE) {
        if (role == DG_GAN_G_FAKE) return x != x ? x : -1.f;
        if (role == DG_GAN_D_REAL) return x < 1.f ? -1.f : (x >= 1.f ? 0.f : x);
        return x > -1.f ? 1.f : (x <= -1.f ? 0.f : x);
    }
    const float e = expf(-fabsf(x));
    const float big = 1.f / (1.f + e), small = e / (1.f + e);               // sigmoid(|x|), sigmoid(-|x|)
    if (tau == 1.f) return x >= 0.f ? -small : -big;                        // -sigmoid(-x)
    const float sig = x >= 0.f ? big : small;                               // sigmoid(x)
    return tau == 0.f ? sig : sig - tau;
}

__global__ __launch_bounds__(256) void gan_loss_fwd_kernel(const DgPtrs xs, int n, int kind, const DgGanRoles roles, float real_label,
                                                           const DgPtrs losses) {
    const float* __restrict__ x = dg_pick<const float>(xs, blockIdx.x);
    float* __restrict__ loss = dg_pick<float>(losses, blockIdx.x);
    const int role = roles.v[blockIdx.x];
    const float tau = gan_tau(role, real_label);
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)gan_term(kind, role, tau, x[i]);
    dg_block_stage_d(s, red);
    if (threadIdx.x == 0) loss[0] = (float)(dg_sum4_seq(red) / n);
}

__global__ __launch_bounds__(256) void gan_loss_bwd_kernel(const DgPtrs xs, int n, int kind, const DgGanRoles roles, float real_label,
                                                           const DgPtrs gouts, const DgPtrs dxs) {
    const float* __restrict__ x = dg_pick<const float>(xs, blockIdx.y);
    const float* __restrict__ gout = dg_pick<const float>(gouts, blockIdx.y);
    float* __restrict__ dx = dg_pick<float>(dxs, blockIdx.y);
    const int role = roles.v[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    dx[i] = gout[0] * gan_deriv(kind, role, gan_tau(role, real_label), x[i]) / (float)n;
}

// the checks both passes share; tabs: the pointer tables, each with `groups` non-null entries.  Fills the by-value role table.
static int gan_check(const char* who, int groups, int n, int kind, const int* role, float real_label, const void* const* const* tabs, int ntabs,
                     DgGanRoles* roles) {
    DG_CHECK_ARG(groups >= 1 && groups <= DG_MAX_GROUPS, "%s: groups=%d (1..%d)", who, groups, DG_MAX_GROUPS);
    for (int k = 0; k < ntabs; ++k) {
        DG_CHECK_ARG(tabs[k] != nullptr, "%s: null pointer table", who);
        for (int i = 0; i < groups; ++i) DG_CHECK_ARG(tabs[k][i] != nullptr, "%s: null pointer (problem %d)", who, i);
    }
    DG_CHECK_ARG(n >= 1, "%s: n=%d (>= 1)", who, n);
    DG_CHECK_ARG(kind == DG_GAN_BCE_LOGITS || kind == DG_GAN_LSGAN || kind == DG_GAN_HINGE, "%s: unknown kind %d", who, kind);
    DG_CHECK_ARG(role != nullptr, "%s: null role table", who);
    for (int i = 0; i < DG_MAX_GROUPS; ++i) {
        roles->v[i] = i < groups ? role[i] : DG_GAN_D_REAL;
        DG_CHECK_ARG(roles->v[i] == DG_GAN_D_REAL || roles->v[i] == DG_GAN_D_FAKE || roles->v[i] == DG_GAN_G_FAKE,
                     "%s: unknown role %d (problem %d)", who, roles->v[i], i);
    }
    DG_CHECK_ARG(isfinite(real_label) && real_label > 0.5f && real_label <= 1.f, "%s: real_label=%g (finite, in (0.5, 1])", who, (double)real_label);
    DG_CHECK_ARG(kind != DG_GAN_HINGE || real_label == 1.f, "%s: the hinge objective takes real_label 1, got %g", who, (double)real_label);
    return DG_OK;
}
#define GAN_TAB(x) ((const void* const*)(x))

extern "C" int dg_gan_loss_fwd_g(int groups, const float* const* logit, int n, int kind, const int* role, float real_label, float* const* loss,
                                 dg_stream_t stream) {
    const void* const* tabs[] = {GAN_TAB(logit), GAN_TAB(loss)};
    DgGanRoles roles;
    const int rc = gan_check("dg_gan_loss_fwd", groups, n, kind, role, real_label, tabs, 2, &roles);
    if (rc != DG_OK) return rc;
    hipLaunchKernelGGL(gan_loss_fwd_kernel, dim3(groups), dim3(256), 0, (hipStream_t)stream, dg_ptrs(GAN_TAB(logit), groups), n, kind, roles,
                       real_label, dg_ptrs(GAN_TAB(loss), groups));
    DG_CHECK_LAUNCH("gan_loss_fwd");
    return DG_OK;
}
extern "C" int dg_gan_loss_fwd(const float* logit, int n, int kind, int role, float real_label, float* loss, dg_stream_t stream) {
    return dg_gan_loss_fwd_g(1, &logit, n, kind, &role, real_label, &loss, stream);
}
extern "C" int dg_gan_loss_bwd_g(int groups, const float* const* logit, int n, int kind, const int* role, float real_label,
                                 const float* const* gout, float* const* dlogit, dg_stream_t stream) {
    const void* const* tabs[] = {GAN_TAB(logit), GAN_TAB(gout), GAN_TAB(dlogit)};
    DgGanRoles roles;
    const int rc = gan_check("dg_gan_loss_bwd", groups, n, kind, role, real_label, tabs, 3, &roles);
    if (rc != DG_OK) return rc;
    hipLaunchKernelGGL(gan_loss_bwd_kernel, dim3((n - 1) / 256 + 1, groups), dim3(256), 0, (hipStream_t)stream, dg_ptrs(GAN_TAB(logit), groups), n,
                       kind, roles, real_label, dg_ptrs(GAN_TAB(gout), groups), dg_ptrs(GAN_TAB(dlogit), groups));
    DG_CHECK_LAUNCH("gan_loss_bwd");
    return DG_OK;
}
extern "C" int dg_gan_loss_bwd(const float* logit, int n, int kind, int role, float real_label, const float* gout, float* dlogit,
                               dg_stream_t stream) {
    return dg_gan_loss_bwd_g(1, &logit, n, kind, &role, real_label, &gout, &dlogit, stream);
}
