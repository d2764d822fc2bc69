// bf_cal.cpp -- the gain solver and the calibrated weights (include/dsabf.h: bf_solve_gains_device, bf_calibrate_weights_device, bf_cal_*;
// contract and measurements: docs/CALIBRATION.md).  The device code is csrc/cal/bf_cal.hip; this file checks the arguments.  Neither call
// keeps anything in the handle: the solver reads the visibilities where they are, so calls on any queues share no memory.
#include "bf_runtime_internal.h"
#include "cal/bf_cal_kernels.h"

static int check_ant(const bf_handle* h, const char* who)
{
    if (!dsabf::cal_supported(h->cfg.n_ant))
        return fail(BF_ERR_INVALID, "%s: %d antennas; the gain solver is defined for multiples of 4 up to %d", who, h->cfg.n_ant, dsabf::kCalMaxAnt);
    return BF_OK;
}

extern "C" {

int bf_cal_default_options(bf_cal_options* o)
{
    if (!o) return fail(BF_ERR_INVALID, "bf_cal_default_options: NULL argument");
    o->tol = 1e-10;
    o->max_iter = 200;
    o->ref_ant = -1;
    o->joint_pol = 0;
    return BF_OK;
}

size_t bf_cal_gain_entries(const bf_config* cfg, int joint_pol)
{
    if (!cfg || cfg->n_freq <= 0 || cfg->n_pol <= 0 || cfg->n_ant <= 0) return 0;
    return (size_t)(joint_pol ? 1 : cfg->n_pol) * (size_t)cfg->n_freq * (size_t)cfg->n_ant;
}

int bf_solve_gains_device(bf_handle* h, const int64_t* d_vis, const double* d_model, const uint8_t* d_flags, const bf_cal_options* opt,
                          double* d_gains, int32_t* d_info, void* hip_stream)
{
    if (!h || !d_vis || !opt || !d_gains || !d_info) return fail(BF_ERR_INVALID, "bf_solve_gains_device: NULL argument");
    if (int rc = check_ant(h, "bf_solve_gains_device")) return rc;
    if (opt->max_iter < 1) return fail(BF_ERR_INVALID, "bf_solve_gains_device: max_iter must be at least 1");
    if (!(opt->tol >= 0.0)) return fail(BF_ERR_INVALID, "bf_solve_gains_device: tol must not be negative");
    if (opt->ref_ant < -1 || opt->ref_ant >= h->cfg.n_ant)
        return fail(BF_ERR_INVALID, "bf_solve_gains_device: ref_ant %d is not an antenna of %d (-1: the first unflagged one)", opt->ref_ant, h->cfg.n_ant);
    if (((uintptr_t)d_vis & 15) || ((uintptr_t)d_model & 15) || ((uintptr_t)d_gains & 15) || ((uintptr_t)d_info & 3))
        return fail(BF_ERR_INVALID, "misaligned device pointer: d_vis, d_model and d_gains must be 16-byte aligned, d_info 4-byte aligned");
    ON_DEVICE(h);
    hipStream_t q = as_stream(hip_stream);
    if (opt->ref_ant >= 0 && d_flags) {   // the one flag the host has to know: read behind whatever hip_stream holds
        uint8_t flagged = 0;
        HIP_TRY(hipMemcpyAsync(&flagged, d_flags + opt->ref_ant, 1, hipMemcpyDeviceToHost, q));
        HIP_TRY(hipStreamSynchronize(q));
        if (flagged) return fail(BF_ERR_INVALID, "bf_solve_gains_device: ref_ant %d is flagged", opt->ref_ant);
    }
    HIP_TRY(dsabf::launch_solve_gains(h->cfg.n_ant, h->cfg.n_freq, h->cfg.n_pol, (const long long*)d_vis, d_model, d_flags, opt->tol, opt->max_iter,
                                      opt->ref_ant, opt->joint_pol != 0, !h->cal_resident, d_gains, d_info, q));
    return BF_OK;
}

int bf_calibrate_weights_device(bf_handle* h, const int8_t* d_w_in, const double* d_gains_layer, const uint8_t* d_flags, int mode, int8_t* d_w_out,
                                void* hip_stream)
{
    if (!h || !d_w_in || !d_gains_layer || !d_w_out) return fail(BF_ERR_INVALID, "bf_calibrate_weights_device: NULL argument");
    if (int rc = check_ant(h, "bf_calibrate_weights_device")) return rc;
    if (mode != BF_CAL_PHASE && mode != BF_CAL_FULL)
        return fail(BF_ERR_INVALID, "bf_calibrate_weights_device: mode %d is neither BF_CAL_PHASE nor BF_CAL_FULL", mode);
    if (((uintptr_t)d_w_in & 3) || ((uintptr_t)d_w_out & 3) || ((uintptr_t)d_gains_layer & 15))
        return fail(BF_ERR_INVALID, "misaligned device pointer: the weight arrays must be 4-byte aligned, d_gains_layer 16-byte aligned");
    ON_DEVICE(h);
    HIP_TRY(dsabf::launch_calibrate_weights(h->cfg.n_ant, h->cfg.n_freq, h->cfg.n_beams, d_w_in, d_gains_layer, d_flags, mode, d_w_out,
                                            as_stream(hip_stream)));
    return BF_OK;
}

}  // extern "C"
