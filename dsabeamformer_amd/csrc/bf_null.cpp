// bf_null.cpp -- the spatial null: interferer vectors from visibilities and the projected weights (include/dsabf.h: bf_null_solve_device,
// bf_null_weights_device, bf_null_*; contract and measurements: docs/NULLING.md).  The device code is csrc/null/bf_null.hip; this file
// checks the arguments.  Neither call keeps anything in the handle: the solver reads the visibilities where they are, so calls on any
// queues share no memory.
#include "bf_runtime_internal.h"
#include "null/bf_null_kernels.h"

static_assert(BF_NULL_MAX == dsabf::kNullMaxVecs, "include/dsabf.h and null/bf_null_kernels.h name the same limit");

static int check_ant(const bf_handle* h, const char* who)
{
    if (!dsabf::null_supported(h->cfg.n_ant))
        return fail(BF_ERR_INVALID, "%s: %d antennas; the spatial null is defined for multiples of 4 up to %d", who, h->cfg.n_ant, dsabf::kNullMaxAnt);
    return BF_OK;
}

extern "C" {

int bf_null_default_options(bf_null_options* o)
{
    if (!o) return fail(BF_ERR_INVALID, "bf_null_default_options: NULL argument");
    o->min_ratio = 4.0;
    o->tol = 1e-6;
    o->n_null = 1;
    o->max_iter = 200;
    o->pol = -1;
    return BF_OK;
}

size_t bf_null_vec_entries(const bf_config* cfg, int n_null)
{
    if (!cfg || cfg->n_freq <= 0 || cfg->n_ant <= 0 || n_null < 1 || n_null > BF_NULL_MAX) return 0;
    return (size_t)cfg->n_freq * (size_t)n_null * (size_t)cfg->n_ant;
}

int bf_null_solve_device(bf_handle* h, const int64_t* d_vis, const uint8_t* d_flags, const bf_null_options* opt, double* d_vecs, double* d_eig,
                         int32_t* d_info, void* hip_stream)
{
    if (!h || !d_vis || !opt || !d_vecs || !d_eig || !d_info) return fail(BF_ERR_INVALID, "bf_null_solve_device: NULL argument");
    if (int rc = check_ant(h, "bf_null_solve_device")) return rc;
    if (opt->n_null < 1 || opt->n_null > BF_NULL_MAX)
        return fail(BF_ERR_INVALID, "bf_null_solve_device: n_null %d is outside 1 ... %d", opt->n_null, BF_NULL_MAX);
    if (opt->max_iter < 1) return fail(BF_ERR_INVALID, "bf_null_solve_device: max_iter must be at least 1");
    if (!(opt->tol >= 0.0)) return fail(BF_ERR_INVALID, "bf_null_solve_device: tol must not be negative");
    if (!(opt->min_ratio >= 0.0)) return fail(BF_ERR_INVALID, "bf_null_solve_device: min_ratio must not be negative");
    if (opt->pol < -1 || opt->pol >= h->cfg.n_pol)
        return fail(BF_ERR_INVALID, "bf_null_solve_device: pol %d is not a polarisation of %d (-1: their sum)", opt->pol, h->cfg.n_pol);
    if (((uintptr_t)d_vis & 15) || ((uintptr_t)d_vecs & 15) || ((uintptr_t)d_eig & 7) || ((uintptr_t)d_info & 3))
        return fail(BF_ERR_INVALID, "misaligned device pointer: d_vis and d_vecs must be 16-byte aligned, d_eig 8-byte, d_info 4-byte aligned");
    ON_DEVICE(h);
    HIP_TRY(dsabf::launch_null_solve(h->cfg.n_ant, h->cfg.n_freq, h->cfg.n_pol, (const long long*)d_vis, d_flags, opt->n_null, opt->min_ratio, opt->tol,
                                     opt->max_iter, opt->pol, !h->null_resident, d_vecs, d_eig, d_info, as_stream(hip_stream)));
    return BF_OK;
}

int bf_null_weights_device(bf_handle* h, const int8_t* d_w_in, const double* d_vecs, const int32_t* d_info, int n_null, const uint8_t* d_flags,
                           int mode, int8_t* d_w_out, double* d_scale, void* hip_stream)
{
    if (!h || !d_w_in || !d_vecs || !d_info || !d_w_out) return fail(BF_ERR_INVALID, "bf_null_weights_device: NULL argument");
    if (int rc = check_ant(h, "bf_null_weights_device")) return rc;
    if (n_null < 1 || n_null > BF_NULL_MAX) return fail(BF_ERR_INVALID, "bf_null_weights_device: n_null %d is outside 1 ... %d", n_null, BF_NULL_MAX);
    if (mode != BF_NULL_SCALED && mode != BF_NULL_CLIP)
        return fail(BF_ERR_INVALID, "bf_null_weights_device: mode %d is neither BF_NULL_SCALED nor BF_NULL_CLIP", mode);
    if (((uintptr_t)d_w_in & 3) || ((uintptr_t)d_w_out & 3) || ((uintptr_t)d_vecs & 15) || ((uintptr_t)d_info & 3) || ((uintptr_t)d_scale & 7))
        return fail(BF_ERR_INVALID,
                    "misaligned device pointer: the weight arrays and d_info must be 4-byte aligned, d_vecs 16-byte, d_scale 8-byte aligned");
    ON_DEVICE(h);
    HIP_TRY(dsabf::launch_null_weights(h->cfg.n_ant, h->cfg.n_freq, h->cfg.n_beams, d_w_in, d_vecs, d_info, n_null, d_flags, mode, d_w_out, d_scale,
                                       as_stream(hip_stream)));
    return BF_OK;
}

}  // extern "C"
