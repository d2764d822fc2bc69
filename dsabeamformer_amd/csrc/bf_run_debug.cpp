// bf_run_debug.cpp -- host mirror, part 3: the DEBUG branch of the reference's main loop (src/beamformer.cu:364-534) on the C-ABI of
// dsabf.h, run_debug_observation.
#include <algorithm>
#include <cstring>
#include <iostream>

#include "../../include/dsabf_host.h"
#include "bf_host_internal.h"
#include "bf_loop_internal.h"

namespace dsabf {
namespace {

// ---- the DEBUG main() flow (src/beamformer.cu:12-621 with -DDEBUG) ----------------------------------------------------
// Block-granular analysis: one fused launch over the block's gemm-units, their detected powers to the host in ONE copy (a4: every
// unit still travels, as src/beamformer.cu:485-488 has it), one DM-0 launch for all of them (a8).
int debug_block_launch(bf_handle* h, const bf_config& cfg, int q, observation_loop_state& obs_state, int n_src, float* beam_out_blk,
                       float* dedispersed_out, bool verbose, std::ostream& log)
{
    const int first_gemm = (int)obs_state.get_current_analysis_gemm(0);
    if (verbose) log << "Queueing Beamforming. Start Dir = " << first_gemm << std::endl;
    const size_t n_f_per_detect = bf_floats_per_detect(&cfg);
    std::vector<float*> dst((size_t)cfg.n_gemms_per_block);
    for (int u = 0; u < cfg.n_gemms_per_block; u++) dst[(size_t)u] = beam_out_blk + n_f_per_detect * (size_t)u;
    int rc = bf_enqueue_block(h, q, (int)obs_state.get_next_gpu_analysis_block(), 0, cfg.n_gemms_per_block, dst.data());
    const int n_valid = std::min(cfg.n_gemms_per_block, n_src - first_gemm);   // check_ready_for_dh2_transfer, :492
    if (rc == BF_OK && n_valid > 0)
        rc = bf_enqueue_block_dedisperse(h, q, 0, n_valid, &dedispersed_out[(size_t)first_gemm * cfg.n_beams]);
    if (rc != BF_OK) return gpu_error(log, rc);
    (void)obs_state.get_current_analysis_gemm(cfg.n_gemms_per_block - 1);   // most_recent_gemm = the block's last unit
    return BF_OK;
}

}  // namespace

int run_debug_observation(const bf_config& cfg, const debug_run_options& opt, debug_run_result* res,
                          std::vector<float>* dedispersed_result, std::ostream& log)
{
    const int n_streams = cfg.n_streams;
    if (cfg.n_gemms_per_block % n_streams) {
        log << "N_GEMMS_PER_BLOCK must be divisible by N_STREAMS" << std::endl;
        return BF_ERR_INVALID;
    }
    if (kSourcesPerBatch % cfg.n_gemms_per_block) {  // static_assert src/beamformer.hh:151
        log << "N_SOURCES_PER_BATCH must be divisible by N_GEMMS_PER_BLOCK" << std::endl;
        return BF_ERR_INVALID;
    }
    std::vector<antenna> pos((size_t)cfg.n_ant);
    std::vector<beam_direction> dir((size_t)cfg.n_beams);
    test_data_generator input_data_generator(cfg);
    if (!input_data_generator.get_data()) return BF_ERR_DEVICE;
    if (opt.sources && input_data_generator.read_in_source_directions(opt.sources) != 0) {
        log << "beam: could not read source direction file " << opt.sources << std::endl;
        return BF_ERR_INVALID;
    }
    if (opt.positions && read_in_position_locations(opt.positions, cfg.n_ant, pos.data()) != 0) return BF_ERR_INVALID;
    if (opt.directions && read_in_beam_directions(opt.directions, cfg.n_beams, dir.data()) != 0) return BF_ERR_INVALID;
    if (!opt.positions) default_positions(cfg.n_ant, pos.data());      // :135-140
    if (!opt.directions) default_directions(cfg.n_beams, dir.data());  // :142-147
    if (opt.verbose) print_all_defines(cfg, log);

    run_device dev;
    int rc = bf_create(&cfg, opt.device, &dev.h);
    if (rc != BF_OK) return gpu_error(log, rc);
    bf_handle* const h = dev.h;

    const int n_src = input_data_generator.get_n_pt_sources();
    const size_t n_f_per_detect = bf_floats_per_detect(&cfg);
    const size_t n_dedispersed = (size_t)cfg.n_beams * std::max(n_src, 1);
    float *beam_out = nullptr, *dedispersed_out = nullptr;
    if ((rc = dev.alloc_pinned(n_f_per_detect * n_streams, &beam_out)) != BF_OK) return rc;  // :249
    if ((rc = dev.alloc_pinned(n_dedispersed, &dedispersed_out)) != BF_OK) return rc;         // :212
    ::memset(dedispersed_out, 0, n_dedispersed * sizeof(float));

    {  // :230-241, :251, :272
        std::vector<int8_t> fourier_coefficients((size_t)cfg.n_freq * cfg.n_ant * cfg.n_beams * 2);
        generate_fourier_coefficients(cfg.n_beams, cfg.n_ant, cfg.n_freq, 0, opt.gpu, pos.data(), dir.data(),
                                      fourier_coefficients.data());
        rc = set_run_weights(h, opt.device, fourier_coefficients, opt.gains, opt.nulls, opt.ant_flags, opt.weights_out, log);
        if (rc != BF_OK) return gpu_error(log, rc);
    }

    std::vector<int> timeSlice((size_t)n_streams);
    for (int i = 0; i < n_streams; i++) timeSlice[i] = i;  // :319
    float* beam_out_blk[2] = {nullptr, nullptr};   // block_launch: a block's detected powers on the host, per alternating queue
    uint64_t block_launches = 0;
    for (int q = 0; q < 2 && opt.block_launch; q++) {   // (page-locking 2 x N_GEMMS_PER_BLOCK x 2 MiB is setup, like beam_out)
        if ((rc = dev.alloc_pinned(n_f_per_detect * (size_t)cfg.n_gemms_per_block, &beam_out_blk[q])) != BF_OK) return rc;
        float* d_blk = nullptr;                        // and the queue's device-side block buffer (allocated at first use otherwise)
        if ((rc = bf_block_output_device(h, q % n_streams, &d_blk)) != BF_OK) return rc;
    }

    hip_backend backend(h);
    observation_loop_state obs_state(kMaxTransferSep, kMaxTotalSep, cfg, &backend, /*debug_mode=*/true);  // :322
    obs_state.set_n_pt_sources(n_src);                                                                  // :325

    if (opt.verbose) {
        log << "Executing beamformer.cu" << "\n";
        log << "MAX_TOTAL_SEP: " << kMaxTotalSep << "\n";
        log << "MAX_TRANSFER_SEP: " << kMaxTransferSep << std::endl;
    }

    float time_accumulator_ms = 0, observation_time_ms = 0;
    bf_timer_start(h);  // :358
    const size_t block_bytes = bf_bytes_per_block(&cfg);
    const size_t input_data_size = input_data_generator.input_data_size();

    while (!obs_state.check_observations_complete()) {  // :364
        if (opt.verbose) log << "##########################################" << std::endl << obs_state << std::endl;
        if (obs_state.check_ready_for_transfer()) {  // :378
            if (input_data_generator.check_need_to_generate_more_input_data((int)obs_state.get_blocks_transferred())) {
                log << "Generating new source data" << std::endl;
                bf_timer_stop(h, &time_accumulator_ms);  // :408-409
                observation_time_ms += time_accumulator_ms;
                input_data_generator.generate_test_data(pos.data(), opt.gpu);
                bf_timer_start(h);
                log << "done generating test data" << std::endl;
            }
            if (input_data_generator.check_data_ready_for_transfer((int)obs_state.get_blocks_transfer_queue())) {  // :421
                char* input_data = input_data_generator.get_data();
                rc = bf_submit_block(h, (int)obs_state.get_next_gpu_transfer_block(),
                                     &input_data[(block_bytes * obs_state.get_blocks_transfer_queue()) % input_data_size],
                                     block_bytes, nullptr);  // :425-429
                if (rc != BF_OK) return gpu_error(log, rc);
                obs_state.generate_transfer_event();  // :431
            }
            obs_state.check_transfers_complete();  // :438
        }
        obs_state.check_transfer_events();  // :446

        if (obs_state.check_ready_for_analysis()) {  // :452
            if (opt.block_launch) {
                // Two queues alternate so that block i+1's kernel overlaps block i's copy.
                const int q = (int)(block_launches++ % 2) % n_streams;
                rc = debug_block_launch(h, cfg, q, obs_state, n_src, beam_out_blk[q], dedispersed_out, opt.verbose, log);
            } else {
                const auto dedisperse_unit = [&](int st, int unit) {
                    if (!obs_state.check_ready_for_dh2_transfer(unit)) return (int)BF_OK;  // :492
                    const int current_gemm = (int)obs_state.get_current_analysis_gemm(unit);
                    if (opt.verbose) log << "Current GEMM: " << current_gemm << std::endl;
                    return bf_enqueue_dedisperse(h, st, &dedispersed_out[(size_t)current_gemm * cfg.n_beams]);  // :498-510
                };
                rc = enqueue_block_by_units(h, cfg, (int)obs_state.get_next_gpu_analysis_block(), timeSlice, log, dedisperse_unit, [&](int st, int unit) {
                    if (opt.verbose && st == 0) log << "Queueing Beamforming. Start Dir = " << obs_state.get_current_analysis_gemm(unit) << std::endl;
                    return &beam_out[(size_t)st * n_f_per_detect];
                });
            }
            if (rc != BF_OK) return rc;
            obs_state.generate_analysis_event();  // :525
        }
        obs_state.check_analysis_events();  // :532
        if (obs_state.status() != BF_OK) return event_backend_error(log, obs_state);
    }

    bf_timer_stop(h, &time_accumulator_ms);  // :540
    observation_time_ms += time_accumulator_ms;
    const long long chunks = (long long)n_src * cfg.n_out_per_gemm;
    const double rate = bf_bytes_per_gemm(&cfg) * (double)n_src / observation_time_ms / 1e6;
    bf_stream_sync(h, -1);  // :560-562
    closing_report(log, observation_time_ms, (uint64_t)chunks, observation_time_ms / chunks, rate,
                   opt.block_launch ? "one bf_enqueue_block per PSRDADA block" : kUnitLaunchPattern);

    if (opt.output && opt.output[0])
        if (write_array_to_disk_as_python_file(dedispersed_out, n_src, cfg.n_beams, opt.output) != 0)  // :568-571
            log << "could not write " << opt.output << std::endl;
    if (dedispersed_result) dedispersed_result->assign(dedispersed_out, dedispersed_out + (size_t)n_src * cfg.n_beams);
    if (res) {
        res->observation_time_ms = observation_time_ms;
        res->n_pt_sources = n_src;
        res->data_chunks = chunks;
    }
    return BF_OK;
}

}  // namespace dsabf
