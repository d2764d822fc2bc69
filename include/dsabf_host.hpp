// dsabf_host.hpp -- C++ host-side mirror of the reference's host classes and helpers, on top of the C-ABI
// (include/dsabf.h).  A reference-style main() can include this header, link libdsabf.so and keep its structure:
// same class names, method names, argument meaning and loop semantics as
//   observation_loop_state   src/observation_loop.hh:1-177
//   test_data_generator      src/test_data_generator.hh:11-108
//   antenna / beam_direction src/beamformer.hh:170-213, readers :250-284, python writer :287-311
//   steering weights         src/beamformer.cu:230-241 (inline in the reference's main)
// Differences, on purpose: geometry is runtime (bf_config) instead of #defines; errors are return codes /
// exceptions instead of exit(); the analysis-complete event is recorded behind ALL compute queues (the
// reference records on stream[7] only -- SURVEY.md section 5, latent race 2).
#pragma once

#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <iosfwd>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "dsabf.h"

namespace dsabf {

// ---- reference constants (src/beamformer.hh:45-85) -----------------------------------------------------
constexpr int kBurnIn = 25;            // BURNIN
constexpr double kHalfFov = 3.5;       // HALF_FOV, degrees
constexpr int kNGpus = 8;              // N_GPUS
constexpr int kTotChannels = 2048;     // TOT_CHANNELS
constexpr double kStartF = 1.28;       // START_F (GHz)
constexpr double kEndF = 1.53;         // END_F
constexpr int kZeroPt = 0;             // ZERO_PT
constexpr double kCSpeed = 299792458.0;
constexpr double kPi = 3.14159265358979;
constexpr int kMaxVal = 127;           // MAX_VAL
constexpr int kSigMaxVal = 7;          // SIG_MAX_VAL
constexpr int kMaxTransferSep = 2;     // MAX_TRANSFER_SEP
constexpr int kMaxTotalSep = 4;        // MAX_TOTAL_SEP
constexpr int kSourcesPerBatch = 1024; // N_SOURCES_PER_BATCH
constexpr unsigned char kBogusData = 0x70;  // BOGUS_DATA, src/test_data_generator.hh:8

// src/beamformer.hh:170-213
class antenna {
public:
    float x = 0, y = 0, z = 0;
};
std::istream& operator>>(std::istream& in, antenna& a);
std::ostream& operator<<(std::ostream& out, const antenna& a);

class beam_direction {
public:
    float theta = 0, phi = 0;
    beam_direction() {}
    beam_direction(float th, float ph) : theta(th), phi(ph) {}
};
std::istream& operator>>(std::istream& in, beam_direction& a);
std::ostream& operator<<(std::ostream& out, const beam_direction& a);

// src/beamformer.hh:250-284.  Return 0, or -1 if the file cannot be opened (the reference does not check).
int read_in_beam_directions(const char* file_name, int expected_beams, beam_direction* dir);
int read_in_position_locations(const char* file_name, int n_antennas, antenna* pos);
// src/beamformer.hh:287-311
int write_array_to_disk_as_python_file(const float* data_out, int rows, int cols, const char* output_filename);
// src/beamformer.hh:314-350 (runtime values)
void print_all_defines(const bf_config& cfg, std::ostream& out);
// src/beamformer.hh:222-243
void usage(bool debug_mode, std::ostream& out);

// src/beamformer.cu:135-147: default linear array / beam fan when no -p / -d file is given
void default_positions(int n_antennas, antenna* pos);
void default_directions(int n_beams, beam_direction* dir);

// Channel centre frequencies (GHz), both of the reference's variants (float bw in main(), double macro in the
// generator); integer division gpu*2048/7 kept verbatim.
float channel_frequency_weights(int gpu, int chan);    // src/beamformer.cu:173,233
float channel_frequency_generator(int gpu, int chan);  // src/test_data_generator.hh:72

// src/beamformer.cu:230-241: int8 steering weights, layout [freq][ant][beam]{re,im}; channels chan0 ..
// chan0+n_freq-1 of sub-band `gpu` (chan0 > 0 is how a frequency shard of a multi-GPU job gets its slice).
void generate_fourier_coefficients(int n_beams, int n_antennas, int n_freq, int chan0, int gpu, const antenna* pos,
                                   const beam_direction* dir, int8_t* out);

// ---- test_data_generator (src/test_data_generator.hh:11-108) --------------------------------------------
class test_data_generator {
private:
    bf_config cfg;
    int n_pt_sources = 1024;
    int n_source_batches = 1;
    int source_batch_counter = 0;
    std::vector<beam_direction> sources;
    bool use_source_catalog = false;
    char* data = nullptr;      // pinned (bf_alloc_pinned) when a GPU runtime is present, else plain host memory
    bool pinned = false;
    int n_sources_per_batch;

public:
    explicit test_data_generator(const bf_config& cfg, int n_sources_per_batch = kSourcesPerBatch, bool pin = true);
    ~test_data_generator();
    test_data_generator(const test_data_generator&) = delete;
    test_data_generator& operator=(const test_data_generator&) = delete;

    int get_n_pt_sources() const { return n_pt_sources; }
    char* get_data() const { return data; }
    size_t input_data_size() const;  // INPUT_DATA_SIZE, src/beamformer.hh:150
    int get_source_batch_counter() const { return source_batch_counter; }

    void generate_test_data(const antenna pos[], int gpu);
    int read_in_source_directions(const char* file_name);
    void set_source_directions(const beam_direction* src, int n);  // same effect as the file reader
    bool check_need_to_generate_more_input_data(int blocks_transfered);
    bool check_data_ready_for_transfer(int blocks_transfer_queue);
};

// ---- observation_loop_state (src/observation_loop.hh:1-177) ----------------------------------------------
// Event backend: the real one records/queries bf_event (HIP events); bfh_obs_create_custom (dsabf_host.h) plugs in any
// other implementation through a table of C callbacks (the CPU tests drive the scheduler that way, with no GPU).
// Every operation reports failure: the reference exits inside gpuErrchk (src/beamformer.cuh:19-29); here the error
// becomes the state's sticky status() and the loops return it instead of polling a dead device forever.
struct event_backend {
    virtual ~event_backend() {}
    virtual void* create() = 0;                  // nullptr on failure
    virtual void destroy(void* ev) = 0;
    virtual int record_transfer(void* ev) = 0;   // behind the last bf_submit_block; BF_OK or < 0
    virtual int record_analysis(void* ev) = 0;   // behind all compute queues; BF_OK or < 0
    virtual int query(void* ev) = 0;             // BF_OK done, BF_NOT_READY, < 0 error
};
event_backend* make_hip_event_backend(bf_handle* h);  // caller deletes

// (One difference from the reference, where both are compile-time and N_BLOCKS_ON_GPU 8 > MAX_TOTAL_SEP 4: the two separations
// are held to the ring's size, cfg.n_blocks_on_gpu -- a transfer must never overwrite a slot whose block is still being analysed.)
class observation_loop_state {
private:
    uint64_t blocks_analyzed = 0;
    uint64_t blocks_transferred = 0;
    uint64_t blocks_analysis_queue = 0;
    uint64_t blocks_transfer_queue = 0;
    uint64_t maximum_transfer_seperation;
    uint64_t maximum_total_seperation;
    bool transfers_complete = false;
    std::vector<void*> BlockTransferredSync;  // N_EVENTS_ON_GPU = 5 * N_BLOCKS_ON_GPU, src/beamformer.hh:128
    std::vector<void*> BlockAnalyzedSync;
    int most_recent_gemm = 0;
    int n_pt_sources = 0;
    bool debug_mode;
    bool verbose;
    int n_gemms_per_block, n_blocks_on_gpu, n_events;
    event_backend* ev;
    int error = 0;  // first backend failure (BF_ERR_*), sticky; 0 = BF_OK
    void fail(int code);

public:
    observation_loop_state(uint64_t maximum_transfer_seperation, uint64_t maximum_total_seperation,
                           const bf_config& cfg, event_backend* backend, bool debug_mode);
    ~observation_loop_state();
    observation_loop_state(const observation_loop_state&) = delete;
    observation_loop_state& operator=(const observation_loop_state&) = delete;

    void generate_transfer_event();  // the reference passes the stream; the backend knows the queue
    void generate_analysis_event();
    void check_transfer_events();
    void check_analysis_events();

    uint64_t get_blocks_analyzed() const { return blocks_analyzed; }
    uint64_t get_blocks_transferred() const { return blocks_transferred; }
    uint64_t get_blocks_analysis_queue() const { return blocks_analysis_queue; }
    uint64_t get_blocks_transfer_queue() const { return blocks_transfer_queue; }

    uint64_t get_current_analysis_gemm(int time_slice);
    uint64_t get_current_transfer_gemm() const;
    uint64_t get_next_gpu_analysis_block() const { return blocks_analysis_queue % n_blocks_on_gpu; }
    uint64_t get_next_gpu_transfer_block() const { return blocks_transfer_queue % n_blocks_on_gpu; }

    void set_transfers_complete(bool value) { transfers_complete = value; }
    bool get_transfers_complete() const { return transfers_complete; }

    bool check_ready_for_transfer() const;
    bool check_ready_for_analysis() const;
    bool check_ready_for_dh2_transfer(int time_slice);

    bool check_observations_complete();
    // BF_OK, or the first error any event operation reported (a failed record / create, a query that returned < 0).
    // Once set, no counter advances any more: callers must stop polling and return it.
    int status() const { return error; }
    void set_n_pt_sources(int val) { n_pt_sources = val; }  // DEBUG only in the reference
    bool check_transfers_complete();                        // DEBUG only in the reference

    friend std::ostream& operator<<(std::ostream& out, const observation_loop_state& a);
};

struct null_vectors;   // what `beam -Z` applies (below, with the spatial null)

// ---- the reference's DEBUG main() as a callable (src/beamformer.cu:12-621, `make debug` flow) -------------
struct debug_run_options {
    int gpu = 0;                 // -g
    const char* positions = nullptr;   // -p
    const char* directions = nullptr;  // -d
    const char* sources = nullptr;     // -s
    const char* output = "bin/data.py";
    int device = 0;
    bool verbose = false;
    // launch granularity (as observation_options::block_launch): true = one fused launch, ONE D2H copy of the block's
    // detected powers and one dedisperse launch (bf_enqueue_block + bf_enqueue_block_dedisperse) per block of
    // N_GEMMS_PER_BLOCK sources, alternating between two compute queues; false = the reference's own pattern, per
    // gemm-unit launches + copies round-robin over the N_STREAMS queues (src/beamformer.cu:454-519).  Same data.py.
    bool block_launch = true;
    // -A: one layer of gains, host [freq][ant]{re, im} (read_gains_layer): the steering weights are multiplied by conj(g) / |g| before
    // they are set (set_weights_calibrated).  weights_out (optional, host, the size of the weight array) receives what was set.
    const double* gains = nullptr;
    const uint8_t* ant_flags = nullptr;   // -f with -A: uint8 [n_ant], flagged antennas get zero weights (needs gains)
    int8_t* weights_out = nullptr;
    // -Z: the interferer vectors of one record (read_null_vectors): projected out of the steering weights (BF_NULL_SCALED) before they are set,
    // after the gains if both are given (set_weights_conditioned); ant_flags then holds for both.
    const null_vectors* nulls = nullptr;
};
struct debug_run_result {
    float observation_time_ms = 0;
    int n_pt_sources = 0;
    long long data_chunks = 0;  // n_pt_sources * N_OUTPUTS_PER_GEMM, src/beamformer.cu:544
};
// Runs generate -> H2D -> fused beamform -> dedisperse -> data.py for every source; dedispersed_out (optional)
// receives the [n_pt_sources][n_beams] table that is also written to opt.output.
int run_debug_observation(const bf_config& cfg, const debug_run_options& opt, debug_run_result* res,
                          std::vector<float>* dedispersed_out, std::ostream& log);

// ---- observation (production) mode: src/beamformer.cu:364-534 without -DDEBUG ------------------------------------
// The surface of dada_handler that the observation loop uses (src/dada_handler.hh:15-23).  The real PSRDADA
// implementation needs libpsrdada (not in this build); anything that hands out pinned blocks
// can stand behind this interface.
struct block_source {
    virtual ~block_source() {}
    virtual void read_headers() {}                 // src/dada_handler.hh:66-90
    virtual char* read() = 0;                      // :92-94  next block (the reference blocks on the shm semaphore)
    virtual void close() = 0;                      // :96-98
    virtual bool check_transfers_complete() = 0;   // :100-116 short block => the observation ends
    virtual uint64_t get_block_size() const = 0;
    virtual uint64_t get_bytes_read() const = 0;
    // true if close() lets a producer overwrite the block.  The reference closes the PSRDADA block right after
    // ENQUEUEING the asynchronous H2D copy (src/beamformer.cu:389-401), i.e. while the DMA may still be reading it -- a
    // latent race that a fast writer turns into corrupted voltages.  For such sources the loop waits for the block's
    // transfer event before close() (PSRDADA allows one open block, so the wait cannot be deferred past the next read).
    virtual bool close_releases_block() const { return false; }
};

// In-memory stand-in for `dada_junkdb` (makefile:28-29, README.md:173): a pinned ring of distinct pseudo-random
// blocks, served n_blocks times, then one short (empty) block.
class junk_block_source : public block_source {
    uint64_t block_size, bytes_read = 0, served = 0, n_blocks;
    int ring_blocks;
    char* ring = nullptr;
    bool pinned = false;

public:
    junk_block_source(const bf_config& cfg, uint64_t n_blocks, int ring_blocks = 4, uint64_t seed = 0xD5A);
    ~junk_block_source() override;
    junk_block_source(const junk_block_source&) = delete;
    junk_block_source& operator=(const junk_block_source&) = delete;
    char* read() override;
    void close() override {}
    bool check_transfers_complete() override;
    uint64_t get_block_size() const override { return block_size; }
    uint64_t get_bytes_read() const override { return bytes_read; }
    const char* ring_data() const { return ring; }           // tests: the bytes block i was served from are
    int get_ring_blocks() const { return ring_blocks; }      // ring_data() + (i % ring_blocks) * block_size
    bool ok() const { return ring != nullptr; }
};

// ---- dedispersion beyond DM 0: the formulas of sandbox/Dispersion Theory.ipynb ------------
// Trial ladder of cells 1-2 (double arithmetic, as numpy): appends trials until the first one >= dm_max.
std::vector<double> dm_trials(double dm0 = 0.0, double dm_max = 2000.0, int nchan = 2048, double epsilon = 1.25,
                              double nu_ghz = (1.28 + 1.53) / 2, double chan_bw_mhz = (1.53 - 1.28) / 2048 * 1000,
                              double ti_us = 40.0, double tscat_us = 0.0, double tsamp_us = 131.0);
// Cell 5: delay[dm][f] = (int)(4.15 * dm * (freq_f^-2 - f_ref^-2) / tsamp_ms); freq in GHz (channel_frequency()).
void dm_delays(const double* dms, int n_dm, const float* freq_ghz, int n_freq, double f_ref_ghz, double tsamp_ms,
               int32_t* out);

// dm_split_trials (observation_options): rank r of R takes trials [first, first + count) of an n_dm-trial ladder -- n_dm / R each,
// the first n_dm % R ranks one more; count may be 0 (more ranks than trials).
void dm_trial_share(int n_dm, int world, int rank, int* first, int* count);

// Fills `ring_blocks` consecutive blocks of cfg's block size at `ring` with the junk source's bytes (64-bit xorshift*,
// every nibble code in both halves; depends only on seed, ring_blocks and the block size).
void junk_fill(const bf_config& cfg, int ring_blocks, uint64_t seed, char* ring);

// ---- shared-memory input ring: the PSRDADA stand-in, csrc/bf_shmring.cpp -------------------
constexpr int kMaxRingBlocks = 64;
constexpr size_t kRingHeaderBytes = 4096;   // HDR_SIZE of config/correlator_header_dsaX.txt

class shm_ring {
    struct control;
    control* ctl = nullptr;
    size_t map_bytes = 0;
    shm_ring();

public:
    ~shm_ring();
    shm_ring(const shm_ring&) = delete;
    shm_ring& operator=(const shm_ring&) = delete;
    // `dada_db -k name -n n_blocks -b block_size` (README.md:151-160); header_text: the ASCII header block
    static shm_ring* create(const char* name, uint64_t n_blocks, uint64_t block_size, const char* header_text);
    static shm_ring* attach(const char* name, int timeout_ms = 10000);
    static int unlink(const char* name);    // `dada_db -k name -d`
    char* open_block_write();               // blocks while the ring is full
    void close_block_write(uint64_t bytes); // bytes < block_size: end of data
    char* open_block_read(uint64_t* bytes, uint64_t* block_id);  // blocks while the ring is empty
    void close_block_read();
    uint64_t get_n_blocks() const;
    uint64_t get_block_size() const;
    uint64_t get_header_size() const;
    const char* get_header() const;
    uint64_t get_blocks_written() const;
    uint64_t get_blocks_read() const;
    char* block(uint64_t slot) const;
};

// dada_handler (src/dada_handler.hh:1-177) on the shared-memory ring: same constructor arguments and messages.
class shm_block_source : public block_source {
    shm_ring* ring = nullptr;
    std::ostream& log;
    uint64_t header_size = 0, block_size = 0, bytes_read = 0, block_id = 0, expected_bytes = 0;
    bool registered = false;

public:
    shm_block_source(const char* name, int core, bool pin, std::ostream& log);
    ~shm_block_source() override;
    shm_block_source(const shm_block_source&) = delete;
    shm_block_source& operator=(const shm_block_source&) = delete;
    bool ok() const { return ring != nullptr; }
    bool is_pinned() const { return registered; }
    void expect_block_bytes(uint64_t n) { expected_bytes = n; }  // N_BYTES_PRE_EXPANSION_PER_BLOCK check, :101-103
    bool close_releases_block() const override { return true; }  // the writer reuses the slot as soon as it is closed
    void read_headers() override;
    char* read() override;
    void close() override;
    bool check_transfers_complete() override;
    uint64_t get_block_size() const override { return block_size; }
    uint64_t get_bytes_read() const override { return bytes_read; }
    const char* get_header() const { return ring ? ring->get_header() : ""; }
};

#ifdef DSABF_WITH_PSRDADA
// dada_handler itself (src/dada_handler.hh:1-177) on a real PSRDADA ring -- only in builds made with -DDSABF_WITH_PSRDADA
// against libpsrdada (csrc/bf_dada.cpp).  Same constructor arguments as the reference (name, core, hex key), same
// messages; errors that make the reference exit(-1) make ok() false / the loop's source fail instead.  No psrdada type
// appears here: the hdu and the multilog are kept as opaque pointers.
class dada_block_source : public block_source {
    void* log = nullptr;      // multilog_t*
    void* hdu_in = nullptr;   // dada_hdu_t*
    std::ostream& out;
    uint64_t header_size = 0, block_size = 0, bytes_read = 0, block_id = 0, expected_bytes = 0;
    bool registered = false, failed = false;
    void cleanup();           // dsaX_dbgpu_cleanup, :118-124
    int dbregister();         // dada_cuda_dbregister, :127-158
    int dbunregister();       // dada_cuda_dbunregister, :160-177

public:
    dada_block_source(const char* name, int core, unsigned in_key, std::ostream& log);   // :25-60
    ~dada_block_source() override;                                                        // :62-64
    dada_block_source(const dada_block_source&) = delete;
    dada_block_source& operator=(const dada_block_source&) = delete;
    bool ok() const { return hdu_in != nullptr && !failed; }
    bool is_pinned() const { return registered; }
    void expect_block_bytes(uint64_t n) { expected_bytes = n; }   // N_BYTES_PRE_EXPANSION_PER_BLOCK check, :101-103
    bool close_releases_block() const override { return true; }   // ipcio_close_block_read hands the block back to the writer
    void read_headers() override;                                  // :66-90
    char* read() override;                                         // :92-94
    void close() override;                                         // :96-98
    bool check_transfers_complete() override;                      // :100-116
    uint64_t get_block_size() const override { return block_size; }
    uint64_t get_bytes_read() const override { return bytes_read; }
};
#endif

// ---- detected-stream sink ---------------------------------------------------------------
// The reference copies each gemm-unit's detected powers into beam_out[stream] and the next gemm-unit of that stream
// overwrites them (src/beamformer.cu:485-488); "writing out ... has not yet been implemented" (README.md:149).  A sink
// gives the stream a consumer without changing the loop: the D2H copy of gemm-unit g lands in acquire(g) -- a pinned
// slot of a ring -- and once the analysis event of g's block has been observed (src/observation_loop.hh:100-117) the
// loop commits the block's gemm-units in index order; commit hands the slot to deliver() and frees it.
// Asynchronous sinks (file, shared-memory ring) deliver on a thread of their own, in order: the loop's commit() only
// marks the slot ready, so a slow consumer costs the loop nothing until the slot ring (five PSRDADA blocks of gemm-units)
// is full -- then acquire() waits for the oldest slot, which is the back-pressure a PSRDADA writer applies.
class detected_sink {
    size_t floats_per_gemm;
    uint64_t n_slots;
    float* ring = nullptr;
    bool pinned = false;
    bool async = false;
    uint64_t next_commit = 0, delivered = 0;   // committed by the loop / handed to deliver(); guarded by `m` when async
    bool failed = false, stop = false;
    std::mutex m;
    std::condition_variable work, done;
    std::thread worker;
    void run();

protected:
    virtual bool deliver(uint64_t gemm_index, const float* data, size_t n_floats) = 0;  // in gemm order
    // `count` consecutive gemm-units that are contiguous in the slot ring (an asynchronous sink that has fallen behind is
    // handed everything that is ready at once); the default hands them to deliver() one by one
    virtual bool deliver_many(uint64_t first_gemm, const float* data, size_t n_floats_each, uint64_t count);
    virtual void finish() {}
    void drain_and_stop();   // every derived destructor calls this first: deliver() must not run on a half-destroyed object

public:
    // slots: gemm-units that can be in flight; the loop needs (MAX_TOTAL_SEP + 1) * N_GEMMS_PER_BLOCK
    detected_sink(const bf_config& cfg, uint64_t slots, bool asynchronous = false);
    virtual ~detected_sink();
    detected_sink(const detected_sink&) = delete;
    detected_sink& operator=(const detected_sink&) = delete;
    static uint64_t slots_for(const bf_config& cfg) { return (uint64_t)(kMaxTotalSep + 1) * cfg.n_gemms_per_block; }
    bool ok();
    float* acquire(uint64_t gemm_index);   // nullptr if the slot still holds an uncommitted gemm-unit (or was committed
                                           // already); waits while an asynchronous delivery of its last occupant is pending
    bool commit(uint64_t gemm_index);      // gemm units must be committed in increasing order, each exactly once
    void close()                           // everything committed has been delivered when this returns
    {
        drain_and_stop();
        finish();
    }
    uint64_t get_delivered();
    size_t get_floats_per_gemm() const { return floats_per_gemm; }
};

// Raw file: a 4096-byte ASCII header (PSRDADA style `KEY value` lines, NUL padded) followed by the gemm-units in
// order, each [N_OUTPUTS_PER_GEMM][N_FREQUENCIES][N_BEAMS] little-endian float32 -- i.e. one long [o][f][b] series.
class file_sink : public detected_sink {
    int fd = -1;
    int write_threads = 4;   // a backlog of several gemm-units is written with positional writes from this many threads

protected:
    bool deliver(uint64_t gemm_index, const float* data, size_t n_floats) override;
    bool deliver_many(uint64_t first_gemm, const float* data, size_t n_floats_each, uint64_t count) override;
    void finish() override;

public:
    static constexpr size_t kHeaderBytes = 4096;
    file_sink(const bf_config& cfg, const char* path, int gpu, uint64_t slots = 0);
    ~file_sink() override;
    bool is_open() const { return fd >= 0; }
};

// Hands every gemm-unit to another process through a shared-memory ring (one ring block per gemm-unit, then a short
// block): the output side of the PSRDADA picture the reference left open ("writing out to the PSRDADA buffer has not yet
// been implemented", README.md:149).  The sink creates the ring; a consumer attaches by name and reads until the short
// block; like any PSRDADA writer the loop blocks while the ring is full.
class ring_sink : public detected_sink {
    shm_ring* out = nullptr;
    std::string name;

protected:
    bool deliver(uint64_t gemm_index, const float* data, size_t n_floats) override;
    void finish() override;

public:
    ring_sink(const bf_config& cfg, const char* ring_name, uint64_t ring_blocks, int gpu, uint64_t slots = 0);
    ~ring_sink() override;
    bool is_open() const { return out != nullptr; }
};

// Keeps everything in host memory (tests, small runs).
class memory_sink : public detected_sink {
protected:
    bool deliver(uint64_t, const float* data, size_t n_floats) override
    {
        data_.insert(data_.end(), data, data + n_floats);
        return true;
    }

public:
    std::vector<float> data_;
    memory_sink(const bf_config& cfg, uint64_t slots = 0) : detected_sink(cfg, slots ? slots : slots_for(cfg)) {}
};

// ---- DM-trial dedispersion of the detected stream, as a stage of the loop ------------------------
// The reference collapses frequency inside its loop behind every gemm-unit (src/beamformer.cu:492-511, DM 0 only).  With
// observation_options::dm_delays set, run_observation pushes every analysed block's beam-blocks into a bf_dm_stream
// (include/dsabf.h) on the block's compute queue -- on the gather root, the gathered whole-band rows -- and hands the chunks
// [n_dm][n_t][n_beams] that become complete to a dm_chunk_sink, in time order, once the block's analysis event has fired.
struct dm_chunk_sink {
    virtual ~dm_chunk_sink() {}
    // out[dm][t][b] for t = first_t .. first_t + n_t - 1 (counted from the first beam-block of the observation)
    virtual bool deliver(uint64_t first_t, int n_t, int n_dm, int n_beams, const float* data) = 0;
    virtual void close() {}
};

// File: a 4096-byte ASCII header (`KEY value` lines, NUL padded; N_DM, N_BEAMS, N_FREQUENCIES, MAX_DELAY, the ladder's
// delays are not repeated), then one record per chunk: 32 bytes {uint64 first_t; uint32 n_t, n_dm, n_beams; 12 bytes of
// zeros} followed by n_dm * n_t * n_beams little-endian float32 in [dm][t][beam] order.
class dm_file_sink : public dm_chunk_sink {
    int fd = -1;
    uint64_t written_t = 0, chunks = 0;

public:
    static constexpr size_t kHeaderBytes = 4096;
    static constexpr size_t kRecordBytes = 32;
    dm_file_sink(const bf_config& cfg, int n_freq_total, int n_dm, int max_delay, const char* path, int gpu, int first_trial = 0);
    ~dm_file_sink() override;
    dm_file_sink(const dm_file_sink&) = delete;
    dm_file_sink& operator=(const dm_file_sink&) = delete;
    bool is_open() const { return fd >= 0; }
    bool deliver(uint64_t first_t, int n_t, int n_dm, int n_beams, const float* data) override;
    void close() override;
    uint64_t get_times_written() const { return written_t; }
    uint64_t get_chunks_written() const { return chunks; }
};

// Hands every chunk to another process through a shared-memory ring (the downstream search's input): one ring block per chunk --
// the 32-byte record {uint64 first_t; uint32 n_t, n_dm, n_beams; zeros} followed by [dm][n_t][beam] float32, padded to the block
// size (32 + n_dm * max_rows * n_beams * 4 bytes: chunks emitted before the delay window has filled hold fewer times) -- then a
// short block.  The sink creates the ring; like any PSRDADA writer the loop blocks while the consumer is a whole ring behind.
class dm_ring_sink : public dm_chunk_sink {
    shm_ring* out = nullptr;
    std::string name;
    size_t block_bytes = 0;
    uint64_t chunks = 0;

public:
    dm_ring_sink(const bf_config& cfg, int n_freq_total, int n_dm, int max_delay, int max_rows, const char* ring_name, uint64_t ring_blocks,
                 int gpu, int first_trial = 0);
    ~dm_ring_sink() override;
    dm_ring_sink(const dm_ring_sink&) = delete;
    dm_ring_sink& operator=(const dm_ring_sink&) = delete;
    bool is_open() const { return out != nullptr; }
    bool deliver(uint64_t first_t, int n_t, int n_dm, int n_beams, const float* data) override;
    void close() override;
    uint64_t get_chunks_written() const { return chunks; }
};

// Keeps the chunks in host memory, assembled as one [n_dm][T][n_beams] series on request (tests, small runs).
class dm_memory_sink : public dm_chunk_sink {
public:
    struct chunk {
        uint64_t first_t;
        int n_t, n_dm, n_beams;
        std::vector<float> data;
    };
    std::vector<chunk> chunks;
    bool deliver(uint64_t first_t, int n_t, int n_dm, int n_beams, const float* data) override
    {
        chunks.push_back({first_t, n_t, n_dm, n_beams, std::vector<float>(data, data + (size_t)n_dm * n_t * n_beams)});
        return true;
    }
};

// ---- Single-pulse search behind the DM stage (include/dsabf.h: bf_sps_*; docs/SINGLE_PULSE.md) ------------------------------
// With observation_options::sps_widths > 0 run_observation creates a bf_sps next to the DM stage, attaches it (every chunk is
// searched on the device, on the queue that produced it) and hands each chunk's candidates to a sps_candidate_sink, in time
// order, once the block's analysis event has fired.
struct sps_candidate_sink {
    virtual ~sps_candidate_sink() {}
    virtual bool deliver(const bf_sps_candidate* cands, size_t n) = 0;
    virtual void close() {}
};

// Text file: a `#` header line, then one line per candidate: t_start dm beam width snr peak (dm: the global trial index).
class sps_file_sink : public sps_candidate_sink {
    FILE* fp = nullptr;
    uint64_t written = 0;

public:
    explicit sps_file_sink(const char* path) : fp(fopen(path, "w"))
    {
        if (fp) fprintf(fp, "# t_start dm beam width snr peak\n");
    }
    ~sps_file_sink() override { close(); }
    sps_file_sink(const sps_file_sink&) = delete;
    sps_file_sink& operator=(const sps_file_sink&) = delete;
    bool is_open() const { return fp != nullptr; }
    bool deliver(const bf_sps_candidate* c, size_t n) override
    {
        if (!fp) return false;
        for (size_t i = 0; i < n; i++)
            if (fprintf(fp, "%llu %d %d %d %.17g %.9g\n", (unsigned long long)c[i].t_start, c[i].dm, c[i].beam, c[i].width, c[i].snr, (double)c[i].peak) < 0)
                return false;
        written += n;
        return true;
    }
    void close() override
    {
        if (fp) fclose(fp);
        fp = nullptr;
    }
    uint64_t get_candidates_written() const { return written; }
};

// ---- Events and stamps behind the search (include/dsabf.h: bf_evt_*, bf_dm_stream_cut_host; docs/EVENTS.md) -------------------
// With observation_options::evt set run_observation feeds every collected chunk's candidates to a bf_evt and hands the events that
// close to an event_sink; with a stamp_sink it also cuts the dedispersed stamp of (at most stamp_max_per_deliver of) them out of the
// DM stage's ring and hands each to the stamp_sink.
struct event_sink {
    virtual ~event_sink() {}
    virtual bool deliver(const bf_evt_event* events, size_t n) = 0;
    virtual void close() {}
};

// Text file: a `#` header line, then one line per event:
// t_start dm beam width snr peak n_members n_beams dm_lo dm_hi t_lo t_hi snr_ib flags (the first six: the best member's record).
class event_file_sink : public event_sink {
    FILE* fp = nullptr;
    uint64_t written = 0;

public:
    explicit event_file_sink(const char* path) : fp(fopen(path, "w"))
    {
        if (fp) fprintf(fp, "# t_start dm beam width snr peak n_members n_beams dm_lo dm_hi t_lo t_hi snr_ib flags\n");
    }
    ~event_file_sink() override { close(); }
    event_file_sink(const event_file_sink&) = delete;
    event_file_sink& operator=(const event_file_sink&) = delete;
    bool is_open() const { return fp != nullptr; }
    bool deliver(const bf_evt_event* e, size_t n) override
    {
        if (!fp) return false;
        for (size_t i = 0; i < n; i++)
            if (fprintf(fp, "%llu %d %d %d %.17g %.9g %d %d %d %d %llu %llu %.17g %u\n", (unsigned long long)e[i].best.t_start, e[i].best.dm, e[i].best.beam,
                        e[i].best.width, e[i].best.snr, (double)e[i].best.peak, e[i].n_members, e[i].n_beams, e[i].dm_lo, e[i].dm_hi,
                        (unsigned long long)e[i].t_lo, (unsigned long long)e[i].t_hi, e[i].snr_ib, e[i].flags) < 0)
                return false;
        written += n;
        return true;
    }
    void close() override
    {
        if (fp) fclose(fp);
        fp = nullptr;
    }
    uint64_t get_events_written() const { return written; }
};

// One stamp: the request it was cut for (t0, the GLOBAL trial index, beam), its time binning, the best member's width and S/N, and
// data float32 [n_freq_out][n_bins].
struct stamp_sink {
    virtual ~stamp_sink() {}
    virtual bool deliver(uint64_t t0, int dm, int beam, int tbin, int width, double snr, const float* data, int n_freq_out, int n_bins) = 0;
    virtual void close() {}
};

// File: the 4096-byte ASCII header (`KEY value` lines, NUL padded: CONTENT stamps, DTYPE float32, NFREQ_OUT, NBINS, FBIN, LAYOUT
// freq,time), then one record per stamp: uint64 t0; int32 dm, beam, tbin, width; double snr; the n_freq_out * n_bins floats.
class stamp_file_sink : public stamp_sink {
    FILE* fp = nullptr;
    uint64_t written = 0;
    int n_freq_out, n_bins;

public:
    static constexpr size_t kHeaderBytes = 4096;
    static constexpr size_t kRecordBytes = 32;
    stamp_file_sink(const char* path, int n_freq_out_, int n_bins_, int fbin) : fp(fopen(path, "wb")), n_freq_out(n_freq_out_), n_bins(n_bins_)
    {
        if (!fp) return;
        char header[kHeaderBytes] = {0};
        snprintf(header, sizeof header, "HDR_SIZE 4096\nCONTENT stamps\nDTYPE float32\nNFREQ_OUT %d\nNBINS %d\nFBIN %d\nLAYOUT freq,time\nRECORD_HEADER_BYTES 32\n",
                 n_freq_out, n_bins, fbin);
        if (fwrite(header, 1, sizeof header, fp) != sizeof header) close();
    }
    ~stamp_file_sink() override { close(); }
    stamp_file_sink(const stamp_file_sink&) = delete;
    stamp_file_sink& operator=(const stamp_file_sink&) = delete;
    bool is_open() const { return fp != nullptr; }
    bool deliver(uint64_t t0, int dm, int beam, int tbin, int width, double snr, const float* data, int nf, int nb) override
    {
        if (!fp || nf != n_freq_out || nb != n_bins) return false;
        const int32_t ints[4] = {dm, beam, tbin, width};
        const size_t n = (size_t)nf * (size_t)nb;
        if (fwrite(&t0, 8, 1, fp) != 1 || fwrite(ints, 4, 4, fp) != 4 || fwrite(&snr, 8, 1, fp) != 1 || fwrite(data, sizeof(float), n, fp) != n) return false;
        written++;
        return true;
    }
    void close() override
    {
        if (fp) fclose(fp);
        fp = nullptr;
    }
    uint64_t get_stamps_written() const { return written; }
};

// ---- Voltage cuts of the search's events (include/dsabf.h: bf_vhist_*; docs/VOLTAGE_CUTS.md) ----------------------------------
// With observation_options::vcut_sink set run_observation keeps a voltage history (bf_vhist) beside the handle, pushes every launch's
// units into it and, of the events one feed closes, cuts the dedispersed voltages of (at most vcut_max_per_deliver of) them.
// One cut: the request it was cut for (t0 in SAMPLES, the GLOBAL trial index), the best member's beam, width and S/N, and data: packed
// bytes [n_units][n_freq][S][n_pol][n_ant] -- gemm-units in the input layout, n_bytes of them.
struct voltage_sink {
    virtual ~voltage_sink() {}
    virtual bool deliver(uint64_t t0, int dm, int beam, int width, double snr, const uint8_t* data, size_t n_bytes) = 0;
    virtual void close() {}
};

// File: the 4096-byte ASCII header (`KEY value` lines, NUL padded: CONTENT voltages, DTYPE packed4+4, NANT, NFREQ, NPOL, NAVG, NOUT, UNITS,
// FIRST_CHANNEL, LAYOUT unit,freq,time,pol,ant), then one record per cut: uint64 t0; int32 dm, beam, width; double snr; the UNITS units.
class voltage_file_sink : public voltage_sink {
    FILE* fp = nullptr;
    uint64_t written = 0;
    size_t cut_bytes;

public:
    static constexpr size_t kHeaderBytes = 4096;
    static constexpr size_t kRecordBytes = 28;
    voltage_file_sink(const char* path, const bf_config& cfg, int units, int first_channel)
        : fp(fopen(path, "wb")), cut_bytes((size_t)units * (size_t)cfg.n_freq * (size_t)cfg.n_out_per_gemm * (size_t)cfg.n_avg * (size_t)cfg.n_pol * (size_t)cfg.n_ant)
    {
        if (!fp) return;
        char header[kHeaderBytes] = {0};
        snprintf(header, sizeof header,
                 "HDR_SIZE 4096\nCONTENT voltages\nDTYPE packed4+4\nNANT %d\nNFREQ %d\nNPOL %d\nNAVG %d\nNOUT %d\nUNITS %d\nFIRST_CHANNEL %d\n"
                 "LAYOUT unit,freq,time,pol,ant\nRECORD_HEADER_BYTES 28\n",
                 cfg.n_ant, cfg.n_freq, cfg.n_pol, cfg.n_avg, cfg.n_out_per_gemm, units, first_channel);
        if (fwrite(header, 1, sizeof header, fp) != sizeof header) close();
    }
    ~voltage_file_sink() override { close(); }
    voltage_file_sink(const voltage_file_sink&) = delete;
    voltage_file_sink& operator=(const voltage_file_sink&) = delete;
    bool is_open() const { return fp != nullptr; }
    bool deliver(uint64_t t0, int dm, int beam, int width, double snr, const uint8_t* data, size_t n_bytes) override
    {
        if (!fp || n_bytes != cut_bytes) return false;
        const int32_t ints[3] = {dm, beam, width};
        if (fwrite(&t0, 8, 1, fp) != 1 || fwrite(ints, 4, 3, fp) != 3 || fwrite(&snr, 8, 1, fp) != 1 || fwrite(data, 1, n_bytes, fp) != n_bytes) return false;
        written++;
        return true;
    }
    void close() override
    {
        if (fp) fclose(fp);
        fp = nullptr;
    }
    uint64_t get_cuts_written() const { return written; }
};

// ---- Coherent dedispersion of a file of voltage cuts (include/dsabf.h: bf_stokes_voltages_device, bf_cdd_*; `beam --coherent`;
// docs/COHERENT_DEDISPERSION.md section 5) ---------------------------------------------------------------------------------------
struct voltage_file_header {
    int n_ant = 0, n_freq = 0, n_pol = 0, n_avg = 0, n_out = 0, units = 0, first_channel = 0;
    size_t record_bytes = 0, n_records = 0;   // packed bytes of one cut; whole records in the file
};
// The header of a voltage_file_sink file.  false + *why if it is not one (two polarisations).  No device is touched.
bool read_voltage_header(const char* path, voltage_file_header* out, std::string* why);
// The smallest power of two >= 256 with n_edge <= N / 4; 0 if none <= 4096 exists.
int coherent_fft_length(int n_edge);
struct coherent_options {
    const char* voltages_path = nullptr;   // in: a voltage_file_sink file
    const char* out_path = nullptr;        // out
    double dm_max = 0.0, tsamp_ms = 0.131;  // -M, -T of the run that wrote the cuts: its ladder, and n_avg voltage samples per tsamp
    int n_dm_cap = 0;                      // -N of that run
    int n_fft = 0;                         // 0: per record, coherent_fft_length of its edge
    int n_int = 1, sideband = 1;
    int gpu = 0, device = 0;
    const antenna* pos = nullptr;          // [NANT] and [n_beams]: the weights the run would use
    const beam_direction* dir = nullptr;
    const double* gains = nullptr;         // -A: a layer [freq][ant]{re, im}, or NULL
    const uint8_t* ant_flags = nullptr;
};
constexpr size_t coherent_file_header_bytes = 4096;
constexpr size_t coherent_record_header_bytes = 44;
// Every record of the voltage file: its `beam` as the one follow-up beam, the DM of its global trial, the edge of bf_cdd_edge over the
// file's channels, then bf_stokes_voltages_device -> bf_cdd_stokes_device.  Writes the 4096-byte ASCII header (CONTENT coherent_stokes,
// DTYPE float32, NFREQ, FIRST_CHANNEL, NFFT (0: chosen per record), NINT, SIDEBAND, NTIME, LAYOUT time,freq,iquv) and per record
// uint64 t0; int32 dm, beam, width; double snr; double dm_value; int32 n_edge, n_fft; float32 [NTIME / NINT][NFREQ]{I, Q, U, V}.
// A record with no FFT length <= 4096 for its edge, or shorter than one segment, is left out and counted in the log line.
int coherent_voltage_file(const coherent_options& o, uint64_t* n_written, uint64_t* n_refused, std::ostream& log);

// ---- Faraday synthesis of a file of coherently dedispersed Stokes parameters (include/dsabf.h: bf_rm_*; `beam --faraday`;
// docs/FARADAY.md section 5) -----------------------------------------------------------------------------------------------------
struct coherent_file_header {
    int n_freq = 0, first_channel = 0, n_time = 0, n_int = 0, n_avg = 0;
    size_t n_rows = 0, n_records = 0;   // rows of one record (n_time / n_int); whole records in the file
};
// The header of a coherent_voltage_file file.  false + *why if it is not one, or does not end with a whole record.  No device is touched.
bool read_coherent_header(const char* path, coherent_file_header* out, std::string* why);
struct faraday_options {
    const char* coherent_path = nullptr;   // in: a coherent_voltage_file file
    const char* out_path = nullptr;        // out
    int n_phi = 0;                         // 0: the default grid, +-phi_max of bf_rm_resolution in steps of fwhm / 8, at most 4096 depths
    double phi_lo = 0.0, phi_hi = 0.0;     // n_phi > 0: phi_p = phi_lo + p (phi_hi - phi_lo) / (n_phi - 1)
    int window = 0;                        // rows of the on-pulse window; 0: the record's search width in rows of the file, at least 1
    const uint8_t* chan_mask = nullptr;    // [n_mask], indexed by the channel of the whole band: non-zero masks it (weight 0), or NULL
    int n_mask = 0;
    int gpu = 0, device = 0;
};
constexpr size_t faraday_file_header_bytes = 4096;
constexpr size_t faraday_record_header_bytes = 84;
constexpr int faraday_min_baseline_rows = 8;
// Every record of the file, on the host in double: the series sum_c I[t][c], a boxcar of w rows over it and its FIRST maximum [lo, lo +
// w); the baseline = the mean of the rows outside [lo - w, lo + 2 w) in ascending order, rounded to float32 (a record with fewer than 8
// such rows is left out and counted); row 0 = the mean of the window's rows, rounded to float32.  Then ONE bf_rm_device call over the
// 1 + n_rows rows (row 0, then the file's) with that baseline.  Writes the 4096-byte ASCII header (CONTENT faraday, DTYPE float32, NFREQ,
// FIRST_CHANNEL, NROWS, NPHI, PHI0, DPHI, LAMBDA0_2, FWHM, PHI_MAX, RECORD_HEADER_BYTES 84) and per record uint64 t0; int32 dm, beam,
// width; double snr, dm_value; int32 n_edge, n_fft (the coherent record's header), int32 lo, w; double rm, pa, lin, frac (bf_rm_refine
// of row 0); float32 [NPHI]{re, im} (row 0's spectrum); bf_rm_peak [1 + NROWS].  On any failure the output file is removed again.
int faraday_coherent_file(const faraday_options& o, uint64_t* n_written, uint64_t* n_left_out, std::ostream& log);

// ---- Pulsar folding behind the DM stage (include/dsabf.h: bf_psr_*, bf_dm_stream_attach_folder; docs/PULSAR_FOLDING.md) -------
// With observation_options::n_psr > 0 run_observation creates a bf_psr next to the DM stage, attaches it, dumps whenever
// psr_dump_rows rows or more have been folded (an incomplete integration at the end is dropped) and hands every collected dump to a psr_sink.
// One dump: hits uint64 [n_psr][n_freq][n_bins] and profile float64 [n_psr][n_freq][n_bins][n_beams] of the n_rows rows from first_row.
struct psr_sink {
    virtual ~psr_sink() {}
    virtual bool deliver(uint64_t first_row, uint64_t n_rows, int n_psr, int n_freq, int n_bins, int n_beams, const uint64_t* hits,
                         const double* profile) = 0;
    virtual void close() {}
};

// File: the 4096-byte ASCII header (`KEY value` lines, NUL padded: CONTENT folds, DTYPE float64, NPSR, NFREQ, NBINS, NBEAMS, LAYOUT),
// then one record per dump: uint64 first_row, n_rows; uint32 n_psr, n_freq, n_bins, n_beams; the hits (uint64); the profile (float64).
class psr_file_sink : public psr_sink {
    FILE* fp = nullptr;
    uint64_t written = 0;

public:
    static constexpr size_t kHeaderBytes = 4096;
    static constexpr size_t kRecordBytes = 32;
    psr_file_sink(const char* path, int n_psr, int n_freq, int n_bins, int n_beams) : fp(fopen(path, "wb"))
    {
        if (!fp) return;
        char header[kHeaderBytes] = {0};
        snprintf(header, sizeof header,
                 "HDR_SIZE 4096\nCONTENT folds\nDTYPE float64\nNPSR %d\nNFREQ %d\nNBINS %d\nNBEAMS %d\nLAYOUT hits[psr,freq,bin],profile[psr,freq,bin,beam]\n"
                 "RECORD_HEADER_BYTES 32\n",
                 n_psr, n_freq, n_bins, n_beams);
        if (fwrite(header, 1, sizeof header, fp) != sizeof header) close();
    }
    ~psr_file_sink() override { close(); }
    psr_file_sink(const psr_file_sink&) = delete;
    psr_file_sink& operator=(const psr_file_sink&) = delete;
    bool is_open() const { return fp != nullptr; }
    bool deliver(uint64_t first_row, uint64_t n_rows, int n_psr, int n_freq, int n_bins, int n_beams, const uint64_t* hits, const double* profile) override
    {
        if (!fp || n_psr < 1 || n_freq < 1 || n_bins < 1 || n_beams < 1) return false;
        const uint64_t rows[2] = {first_row, n_rows};
        const uint32_t dims[4] = {(uint32_t)n_psr, (uint32_t)n_freq, (uint32_t)n_bins, (uint32_t)n_beams};
        const size_t n_hits = (size_t)n_psr * (size_t)n_freq * (size_t)n_bins, n_prof = n_hits * (size_t)n_beams;
        if (fwrite(rows, 8, 2, fp) != 2 || fwrite(dims, 4, 4, fp) != 4 || fwrite(hits, 8, n_hits, fp) != n_hits || fwrite(profile, 8, n_prof, fp) != n_prof)
            return false;
        written++;
        return true;
    }
    void close() override
    {
        if (fp) fclose(fp);
        fp = nullptr;
    }
    uint64_t get_dumps_written() const { return written; }
};

// ---- Periodicity search behind the DM stage (include/dsabf.h: bf_ffa_*, bf_dm_stream_attach_periodicity; docs/PERIODICITY.md) ----
// With observation_options::ffa_p_hi > 0 run_observation creates a bf_ffa next to the DM stage, attaches it (every chunk is decimated
// into the stage's series on the queue that produced it; a chunk that completes a segment also searches it) and hands the
// candidates of every segment to an ffa_sink, in segment order, once the block whose chunk completed the segment has been analysed.
struct ffa_sink {
    virtual ~ffa_sink() {}
    virtual bool deliver(const bf_ffa_candidate* cands, size_t n) = 0;
    virtual void close() {}
};

// Text file (docs/PERIODICITY.md section 6): `#` header lines (the search's parameters as key=value words, then the column names),
// then one line per candidate: first_row n_rows period_rows dm beam octave p shift bin width snr value (dm: the global trial index;
// period_rows and snr with 17 significant digits, value with 9: they read back to the same bits).
class ffa_file_sink : public ffa_sink {
    FILE* fp = nullptr;
    uint64_t written = 0;

public:
    // detrend_blk > 0 (the stage's bf_ffa_set_detrend) appends ` detrend=blk:win` to the first line; 0 leaves it as it always was
    ffa_file_sink(const char* path, int tdec, int n_seg, int n_oct, int p_lo, int p_hi, int n_widths, double threshold, int detrend_blk = 0,
                  int detrend_win = 0)
        : fp(fopen(path, "w"))
    {
        if (!fp) return;
        fprintf(fp, "# periodicity tdec=%d n_seg=%d n_oct=%d p_lo=%d p_hi=%d n_widths=%d threshold=%.17g", tdec, n_seg, n_oct, p_lo, p_hi, n_widths, threshold);
        if (detrend_blk > 0) fprintf(fp, " detrend=%d:%d", detrend_blk, detrend_win);
        fprintf(fp, "\n# first_row n_rows period_rows dm beam octave p shift bin width snr value\n");
    }
    ~ffa_file_sink() override { close(); }
    ffa_file_sink(const ffa_file_sink&) = delete;
    ffa_file_sink& operator=(const ffa_file_sink&) = delete;
    bool is_open() const { return fp != nullptr; }
    bool deliver(const bf_ffa_candidate* c, size_t n) override
    {
        if (!fp) return false;
        for (size_t i = 0; i < n; i++)
            if (fprintf(fp, "%llu %llu %.17g %d %d %d %d %d %d %d %.17g %.9g\n", (unsigned long long)c[i].first_row, (unsigned long long)c[i].n_rows,
                        c[i].period_rows, c[i].dm, c[i].beam, c[i].octave, c[i].p, c[i].shift, c[i].bin, c[i].width, c[i].snr, (double)c[i].value) < 0)
                return false;
        written += n;
        return true;
    }
    void close() override
    {
        if (fp) fclose(fp);
        fp = nullptr;
    }
    uint64_t get_candidates_written() const { return written; }
};

// ---- What the int64 record files of the three stages below share (vis_file_sink, sk_file_sink, stokes_file_sink) ---------------
// The 4096-byte ASCII header (`KEY value` lines, NUL padded), then one record per delivery: two uint64, the entries (little-endian
// int64).  A sink supplies the header's CONTENT and LAYOUT and, if it has any, lines of its own (`extra`, in front of the GPU line).
class int64_record_file {
    int fd = -1;
    uint64_t records = 0;

protected:
    int64_record_file(const bf_config& cfg, const char* path, const char* content, const char* layout, int first_channel, const std::string& extra,
                      int gpu);
    ~int64_record_file() { close_file(); }
    bool write_record(uint64_t first, uint64_t count, const int64_t* data, size_t n_int64);
    void close_file();
    uint64_t records_written() const { return records; }

public:
    static constexpr size_t kHeaderBytes = 4096;
    static constexpr size_t kRecordBytes = 16;
    int64_record_file(const int64_record_file&) = delete;
    int64_record_file& operator=(const int64_record_file&) = delete;
    bool is_open() const { return fd >= 0; }
};

// ---- The correlator inside the loop (include/dsabf.h: bf_corr_*; docs/CORRELATOR.md) ------------------------------------------
// With observation_options::corr_blocks > 0 run_observation creates a bf_corr, pushes the gemm-units of every launch into it on the
// launch's queue (behind the detect launch, from the resident block), dumps after the last launch of every corr_blocks-th analysed
// block and hands each dump to a vis_sink once that block's analysis event has fired.
struct vis_sink {
    virtual ~vis_sink() {}
    // one integration: blocks first_block .. first_block + corr_blocks - 1 (counted from the first analysed block), n_columns_per_pol
    // columns per polarisation, vis = int64 [freq][pol][a1 (a1 + 1) / 2 + a2]{re, im} (n_int64 values)
    virtual bool deliver(uint64_t first_block, uint64_t n_columns_per_pol, const int64_t* vis, size_t n_int64) = 0;
    virtual void close() {}
};

// File: the 4096-byte ASCII header (`KEY value` lines, NUL padded: CONTENT visibilities, DTYPE int64, NANT, NPOL, NFREQ,
// FIRST_CHANNEL, LAYOUT freq,pol,baseline(lower triangle a1*(a1+1)/2+a2),reim), then one record per dump: uint64 first_block,
// uint64 n_columns_per_pol, the entries (little-endian int64).
class vis_file_sink : public vis_sink, public int64_record_file {
public:
    vis_file_sink(const bf_config& cfg, const char* path, int first_channel, int gpu);
    bool deliver(uint64_t first_block, uint64_t n_columns_per_pol, const int64_t* vis, size_t n_int64) override
    {
        return write_record(first_block, n_columns_per_pol, vis, n_int64);
    }
    void close() override { close_file(); }
    uint64_t get_dumps_written() const { return records_written(); }
};

// Keeps the dumps in host memory (tests, small runs).
class vis_memory_sink : public vis_sink {
public:
    struct dump {
        uint64_t first_block, n_columns_per_pol;
        std::vector<int64_t> vis;
    };
    std::vector<dump> dumps;
    bool deliver(uint64_t first_block, uint64_t n_columns_per_pol, const int64_t* vis, size_t n_int64) override
    {
        dumps.push_back({first_block, n_columns_per_pol, std::vector<int64_t>(vis, vis + n_int64)});
        return true;
    }
};

// ---- The voltage moments inside the loop (include/dsabf.h: bf_sk_*; docs/SPECTRAL_KURTOSIS.md) ---------------------------------
// With observation_options::sk_blocks > 0 run_observation creates a bf_sk and treats it exactly as the correlator above: a push per
// launch on the launch's queue, a dump after every sk_blocks-th analysed block, each dump handed to a sk_sink once that block's
// analysis event has fired.
struct sk_sink {
    virtual ~sk_sink() {}
    // one integration: blocks first_block .. first_block + sk_blocks - 1, n_columns_per_pol columns per polarisation,
    // moments = int64 [freq][pol][ant]{m1, m2} (n_int64 values)
    virtual bool deliver(uint64_t first_block, uint64_t n_columns_per_pol, const int64_t* moments, size_t n_int64) = 0;
    virtual void close() {}
};

// File: the 4096-byte ASCII header (`KEY value` lines, NUL padded: CONTENT voltage_moments, DTYPE int64, NANT, NPOL, NFREQ,
// FIRST_CHANNEL, LAYOUT freq,pol,ant,m1m2), then one record per dump: uint64 first_block, uint64 n_columns_per_pol, the entries
// (little-endian int64).
class sk_file_sink : public sk_sink, public int64_record_file {
public:
    sk_file_sink(const bf_config& cfg, const char* path, int first_channel, int gpu);
    bool deliver(uint64_t first_block, uint64_t n_columns_per_pol, const int64_t* moments, size_t n_int64) override
    {
        return write_record(first_block, n_columns_per_pol, moments, n_int64);
    }
    void close() override { close_file(); }
    uint64_t get_dumps_written() const { return records_written(); }
};

// ---- Full-Stokes follow-up beams inside the loop (include/dsabf.h: bf_stokes_*; docs/STOKES.md) --------------------------------
// With observation_options::stokes_beams non-empty run_observation creates a bf_stokes, sets its weights from the host weights the
// handle got (the calibrated ones with gains), pushes every launch's units on that launch's queue behind the detect launch and hands
// every collected set to a stokes_sink once the launch's block has been analysed.
struct stokes_sink {
    virtual ~stokes_sink() {}
    // one push: the gemm-units first_unit .. first_unit + n_units - 1, counted from the first analysed block;
    // stokes = int64 [unit][t][freq][beam]{I, Q, U, V} (n_int64 values)
    virtual bool deliver(uint64_t first_unit, uint64_t n_units, const int64_t* stokes, size_t n_int64) = 0;
    virtual void close() {}
};

// File: the 4096-byte ASCII header (`KEY value` lines, NUL padded: CONTENT stokes, DTYPE int64, NANT, NFREQ, FIRST_CHANNEL, NINT, NSEL,
// BEAMS b0,b1,..., LAYOUT unit,time,freq,beam,iquv), then one record per collected set: uint64 first_unit, uint64 n_units, the entries
// (little-endian int64).
class stokes_file_sink : public stokes_sink, public int64_record_file {
public:
    stokes_file_sink(const bf_config& cfg, const char* path, int first_channel, int gpu, const std::vector<int>& beams, int n_int);
    bool deliver(uint64_t first_unit, uint64_t n_units, const int64_t* stokes, size_t n_int64) override
    {
        return write_record(first_unit, n_units, stokes, n_int64);
    }
    void close() override { close_file(); }
    uint64_t get_sets_written() const { return records_written(); }
};

// `beam -b`: a comma-separated list of beam indices -> beams.  false + *why if it is empty, holds anything but indices 0 .. n_beams - 1,
// more than BF_STOKES_MAX_BEAMS of them, or one twice.  No device is touched.
bool parse_beam_list(const char* text, int n_beams, std::vector<int>* beams, std::string* why);

// ---- The gain solver (include/dsabf.h: bf_solve_gains_device, bf_calibrate_weights_device; docs/CALIBRATION.md) ----------------
// Thin wrappers: device pointers in, asynchronous on `stream`, the C-ABI's return codes.
inline int solve_gains(bf_handle* h, const int64_t* d_vis, const double* d_model, const uint8_t* d_flags, const bf_cal_options& opt, double* d_gains,
                       int32_t* d_info, void* stream = nullptr)
{
    return bf_solve_gains_device(h, d_vis, d_model, d_flags, &opt, d_gains, d_info, stream);
}
inline int calibrate_weights(bf_handle* h, const int8_t* d_w_in, const double* d_gains_layer, const uint8_t* d_flags, int mode, int8_t* d_w_out,
                             void* stream = nullptr)
{
    return bf_calibrate_weights_device(h, d_w_in, d_gains_layer, d_flags, mode, d_w_out, stream);
}

// File of gains: the 4096-byte ASCII header (`KEY value` lines, NUL padded: CONTENT gains, DTYPE float64, NANT, NPOL (= pol_out), NFREQ,
// FIRST_CHANNEL, LAYOUT pol,freq,ant,reim), then one record per solve: uint64 first_block, uint64 n_columns_per_pol (those of the
// visibility record it was solved from), the gains (little-endian float64 [pol_out][freq][ant]{re, im}), the info (int32
// [pol_out][freq]{iterations, status}).
class gains_file_sink {
    int fd = -1;
    uint64_t records = 0;
    size_t n_gain_doubles = 0, n_info = 0;

public:
    static constexpr size_t kHeaderBytes = 4096;
    static constexpr size_t kRecordBytes = 16;
    gains_file_sink(int n_ant, int pol_out, int n_freq, int first_channel, const char* path);
    ~gains_file_sink();
    gains_file_sink(const gains_file_sink&) = delete;
    gains_file_sink& operator=(const gains_file_sink&) = delete;
    bool is_open() const { return fd >= 0; }
    bool deliver(uint64_t first_block, uint64_t n_columns_per_pol, const double* gains, const int32_t* info);
    void close();
    uint64_t get_records_written() const { return records; }
};

// The header both record files share (vis_file_sink, gains_file_sink).  read_record_file_header: false + *why if the file cannot be read
// or is neither.  No device is touched.
struct record_file_header {
    std::string content, dtype;
    int n_ant = 0, n_pol = 0, n_freq = 0, first_channel = 0;
    size_t header_bytes = 0, record_header_bytes = 0, file_bytes = 0;
};
bool read_record_file_header(const char* path, record_file_header* out, std::string* why);
// Layer 0 of the LAST record of a gains file, [freq][ant]{re, im}: what `beam -A` applies.  The geometry must be n_ant x n_freq
// starting at first_channel; false + *why otherwise.  No device is touched.
bool read_gains_layer(const char* path, int n_ant, int n_freq, int first_channel, std::vector<double>* layer, std::string* why);
// `beam -E vis_file -G gains_file [-P]`: every record of a vis_file_sink file uploaded, solved with the all-ones model and the default
// options (joint_pol as given) and written as one gains record; the geometry comes from the file's header.
// ant_flags (optional, host, uint8 [NANT of the file]; `beam -f`): non-zero antennas are left out, their gains are exactly (0, 0);
// ref_ant stays -1, the first unflagged antenna.
int solve_vis_file(const char* vis_path, const char* gains_path, bool joint_pol, int device, uint64_t* n_records, std::ostream& log,
                   const uint8_t* ant_flags = nullptr);
// Weights `w` (host, the layout of bf_set_weights) times conj(g) / |g| of one layer of gains (host, [freq][ant]{re, im}), on the device
// (bf_calibrate_weights_device, BF_CAL_PHASE), then set on the handle (bf_set_weights_device); w_set (optional, host) receives them.
// ant_flags (optional, host, uint8 [n_ant]): flagged antennas get zero weights.
int set_weights_calibrated(bf_handle* h, int device, const int8_t* w, const double* gains_layer, int8_t* w_set = nullptr,
                           const uint8_t* ant_flags = nullptr);
// An index file in the format of `beam -F` (one index per line, # comments) -> flags[n] (1 at every index listed).  false + *why if the
// file cannot be read or holds anything but indices 0 .. n - 1.  No device is touched.
bool read_index_file(const char* path, int n, std::vector<uint8_t>* flags, std::string* why);
// The moments file of a sk_file_sink (`beam -Y`): its records SUMMED -- the moments add, and so do the columns per polarisation.
// false + *why if it is not such a file or holds no whole record.  No device is touched.
bool read_moments_sum(const char* path, record_file_header* header, std::vector<int64_t>* moments, uint64_t* n_columns_per_pol, std::string* why);
// `beam -e moments_file -O ant_file [-q chan_file]`: bf_sk_select on the summed records; the flagged antenna indices to ant_path and (if
// given) the flagged channel indices, offset by the file's FIRST_CHANNEL, to chan_path, both in the `-F` format.  No device is touched.
int select_moments_file(const char* moments_path, const bf_sk_options& opt, const char* ant_path, const char* chan_path, std::ostream& log);

// ---- The spatial null (include/dsabf.h: bf_null_solve_device, bf_null_weights_device; docs/NULLING.md) -------------------------
// Thin wrappers: device pointers in, asynchronous on `stream`, the C-ABI's return codes.
inline int null_solve(bf_handle* h, const int64_t* d_vis, const uint8_t* d_flags, const bf_null_options& opt, double* d_vecs, double* d_eig,
                      int32_t* d_info, void* stream = nullptr)
{
    return bf_null_solve_device(h, d_vis, d_flags, &opt, d_vecs, d_eig, d_info, stream);
}
inline int null_weights(bf_handle* h, const int8_t* d_w_in, const double* d_vecs, const int32_t* d_info, int n_null, const uint8_t* d_flags, int mode,
                        int8_t* d_w_out, double* d_scale = nullptr, void* stream = nullptr)
{
    return bf_null_weights_device(h, d_w_in, d_vecs, d_info, n_null, d_flags, mode, d_w_out, d_scale, stream);
}

// File of interferer vectors: the 4096-byte ASCII header (`KEY value` lines, NUL padded: CONTENT nullvecs, DTYPE float64, NANT, NFREQ,
// FIRST_CHANNEL, NNULL, LAYOUT freq,vec,ant,reim; NPOL 1: one set for both polarisations), then one record per solve: uint64 first_block,
// uint64 n_columns_per_pol (those of the visibility record it was solved from), the vectors (little-endian float64
// [freq][n_null][ant]{re, im}), the eigenvalues (float64 [freq][n_null + 1]), the info (int32 [freq][1 + 2 n_null]).
class null_file_sink {
    int fd = -1;
    uint64_t records = 0;
    size_t n_vec_doubles = 0, n_eig = 0, n_info = 0;

public:
    static constexpr size_t kHeaderBytes = 4096;
    static constexpr size_t kRecordBytes = 16;
    null_file_sink(int n_ant, int n_freq, int first_channel, int n_null, const char* path);
    ~null_file_sink();
    null_file_sink(const null_file_sink&) = delete;
    null_file_sink& operator=(const null_file_sink&) = delete;
    bool is_open() const { return fd >= 0; }
    bool deliver(uint64_t first_block, uint64_t n_columns_per_pol, const double* vecs, const double* eig, const int32_t* info);
    void close();
    uint64_t get_records_written() const { return records; }
};
// The vectors and the info of one record, as bf_null_weights_device takes them.
struct null_vectors {
    int n_null = 0;
    std::vector<double> vecs;    // [freq][n_null][ant]{re, im}
    std::vector<int32_t> info;   // [freq][1 + 2 n_null]
};
// The LAST record of a null file: what `beam -Z` applies.  The geometry must be n_ant x n_freq starting at first_channel; false + *why
// otherwise.  No device is touched.
bool read_null_vectors(const char* path, int n_ant, int n_freq, int first_channel, null_vectors* out, std::string* why);
// `beam -E vis_file -Z null_file [-y n_null[:min_ratio]]`: every record of a vis_file_sink file uploaded, solved (bf_null_solve_device with
// opt) and written as one record; the geometry comes from the file's header.  ant_flags (optional, host, uint8 [NANT of the file]).
int null_vis_file(const char* vis_path, const char* null_path, const bf_null_options& opt, int device, uint64_t* n_records, std::ostream& log,
                  const uint8_t* ant_flags = nullptr);
// Weights `w` (host, the layout of bf_set_weights) conditioned on the device and set on the handle (bf_set_weights_device): first times
// conj(g) / |g| of one layer of gains (gains_layer, may be NULL; bf_calibrate_weights_device, BF_CAL_PHASE), then the vectors of `nulls`
// (may be NULL) projected out (bf_null_weights_device, BF_NULL_SCALED) -- the vectors were measured in the antenna domain that the
// calibrated weights address.  w_set (optional, host) receives what was set; ant_flags (optional): zero weights for those antennas.
int set_weights_conditioned(bf_handle* h, int device, const int8_t* w, const double* gains_layer, const null_vectors* nulls, int8_t* w_set = nullptr,
                            const uint8_t* ant_flags = nullptr);

// ---- Pulse injection in front of the DM stage (include/dsabf.h: bf_inj_*, bf_dm_stream_attach_injector; docs/INJECTION.md) -------------
// A plain container: the bursts and trains of a run with their host tables, as bf_inj_add_burst / bf_inj_add_train take them.
// observation_options::inj points at one; run_observation adds the bursts in order (ids 0 ..), then the trains.
struct inj_plan {
    struct burst {
        int64_t t0 = 0;
        int W = 0;
        std::vector<int32_t> delay;    // [band]: one row of dm_delays
        std::vector<float> profile;    // [band][W]
        std::vector<float> response;   // [n_beams]
    };
    struct train {
        bf_psr_model model = {0, 0, 0, 0};
        uint64_t first_row = 0, n_rows = UINT64_MAX;   // UINT64_MAX: until the end
        int n_bins = 0;
        std::vector<int32_t> delay;    // [band]
        std::vector<float> profile;    // [band][n_bins]
        std::vector<float> response;   // [n_beams]
    };
    std::vector<burst> bursts;
    std::vector<train> trains;
    size_t size() const { return bursts.size() + trains.size(); }
};

struct observation_options {
    int gpu = 0;          // -g
    int device = 0;
    int burn_in = 0;      // BURNIN read/close cycles before the loop (src/beamformer.cu:348-355)
    bool verbose = false;
    detected_sink* sink = nullptr;  // optional consumer of every gemm-unit's detected powers; replaces beam_out as
                                    // the D2H destination (beam_out then stays zero)
    // launch granularity: true = bf_enqueue_block launches over `units_per_launch` consecutive gemm-units of the block
    // (0 = the whole PSRDADA block in one launch, the default), consecutive launches on consecutive compute queues, each
    // followed on its queue by the D2H copies of its units (into the sink's slots, or beam_out[queue]); false = the
    // reference's own pattern, one launch per gemm-unit round-robin over the queues (src/beamformer.cu:454-519).
    // Identical detected powers either way.  End to end the loop is PCIe-bound and the granularity does not matter
    // (9.7-10.5 us per beam-block for 1 ... 32 units per launch, profiles/r02_streaming.txt); the whole block per launch
    // is what keeps the kernel at its best rate once the input is resident (profiles/r02_launch_size.txt).
    bool block_launch = true;
    int units_per_launch = 0;
    // -R / -r: this process beamforms frequencies [rank * n_freq, (rank + 1) * n_freq) of a world x n_freq sub-band (cfg.n_freq
    // is the LOCAL count).  The weights are generated for those channels; the input blocks are the rank's own slice.
    int world = 1, rank = 0;
    // Sharded run: the communicator of the frequency partition (bf_comm_create; rank / world above must agree with it).
    // After every block the detected powers of all shards are gathered to rank `gather_root` (BF_GATHER_ROOT_ALL: to every rank) in the reference's
    // [unit][output][freq over the whole band][beam] layout; only that rank copies to the host / feeds `sink` (which
    // must then be built for the whole band: cfg.n_freq * world) -- the others pass sink = nullptr.  Needs block_launch.
    bf_comm* comm = nullptr;
    int gather_root = 0;
    // Transport of that gather (both give the same [unit][o][f over the band][b] on the root): false = every (row, sender) run
    // received in place (bf_gather_detected), true = one message per sender + one device re-layout pass
    // (bf_gather_detected_staged).
    bool gather_staged = false;
    // Sharded run: false if THIS rank's caller failed its own preparations (a sink that did not open, a source that is not there).
    // Every shard exchanges one "ready" flag before the loop; if any is false, all of them return BF_ERR_STATE and nothing is started
    // -- a rank that bails out alone would leave the others waiting in the first gather for ever.  A caller that detects such a
    // failure therefore still CALLS run_observation (with this flag cleared) instead of returning on its own.
    bool local_setup_ok = true;
    // DM-trial dedispersion of the detected stream (needs block_launch): int32 [n_dm][cfg.n_freq * world] sample delays, all >= 0
    // (dm_delays()).  Every analysed block is pushed into a bf_dm_stream behind its launch -- on a sharded run by the gather
    // root, on the gathered band -- and the chunks go to dm_sink (may be NULL: the stage still runs, e.g. for timing).
    const int32_t* dm_delays = nullptr;
    int n_dm = 0;
    dm_chunk_sink* dm_sink = nullptr;
    // Sharded runs only, with gather_root = BF_GATHER_ROOT_ALL (every rank receives the whole band: the ONE collective of the path
    // becomes an all-gather): rank r dedisperses ITS share of the ladder -- trials [r n / R, (r + 1) n / R), the first n % R ranks
    // one more -- so the DM work scales with the GPUs.  Every rank may then have a dm_sink of its own; a chunk carries the rank's
    // trials only (dm_file_sink records the first one as DM_FIRST_TRIAL).
    bool dm_split_trials = false;
    // Single-pulse search of every DM chunk (needs dm_delays): boxcar widths 1 .. 2^(sps_widths-1), 0 = off; candidates at or above
    // sps_threshold (S/N against the mean and deviation of the last 8 chunks) go to sps_sink (may be NULL: the stage still runs),
    // with global trial indices.  With dm_split_trials every rank searches its own trials and may have a sink of its own.
    int sps_widths = 0;
    double sps_threshold = 8.0;
    sps_candidate_sink* sps_sink = nullptr;
    // Events and stamps (docs/EVENTS.md; evt needs sps_widths > 0, stamp_sink needs evt).  evt: the builder's options (NULL = off);
    // max_width is forced to the search's 2^(sps_widths-1), an ib_beam of -1 becomes incoherent_beam.  Closed events go to event_sink
    // (may be NULL).  Of the events ONE FEED closes -- deliver() feeds one collected chunk at a time, so the rule does not depend on how
    // many chunks a deliver happens to find -- at most stamp_max_per_deliver -- by snr descending, then event order; flagged ones only with
    // stamp_flagged -- get a stamp of stamp_bins bins of stamp_tbin samples (0: max(1, best.width / 2)) and stamp_fbin channels per
    // row, centred on the best member; the rest count in observation_result::stamps_dropped.  The DM stage is created with the
    // history of docs/EVENTS.md section 3.  With dm_split_trials every rank builds and cuts its own trials.
    const bf_evt_options* evt = nullptr;
    dsabf::event_sink* event_sink = nullptr;
    dsabf::stamp_sink* stamp_sink = nullptr;
    int stamp_bins = 64;
    int stamp_tbin = 0;
    int stamp_fbin = 1;
    bool stamp_flagged = false;
    int stamp_max_per_deliver = 16;
    // Voltage cuts (docs/VOLTAGE_CUTS.md; vcut_sink needs evt, and so sps_widths > 0 and dm_delays; single-rank runs only): a bf_vhist is
    // created beside the handle with the DM stage's row delays of this rank's trials, in samples (row delay x n_avg: the ladder of
    // the detected stream, nothing finer), and a ring of vcut_history_units units (0: bf_vhist_units_needed).  Every launch's units are
    // pushed on its queue behind the detect.  Of the events ONE FEED closes at most vcut_max_per_deliver -- by snr descending, then event
    // order; flagged ones only with vcut_flagged -- get vcut_units dedispersed units centred on the best member; the rest count in
    // observation_result::vcuts_dropped.
    dsabf::voltage_sink* vcut_sink = nullptr;
    int vcut_units = 2;
    int vcut_history_units = 0;
    bool vcut_flagged = false;
    int vcut_max_per_deliver = 4;
    // Conditioning in front of the DM stage (docs/CONDITIONING.md; needs dm_delays): cond_baseline = pushes of the statistics' window
    // (1 .. 64), 0 = off.  A bf_cond is created next to the DM stage and attached to it: every pushed block is normalised per
    // (channel, beam), masked (cond_mask: host uint8 [cfg.n_freq * world], nonzero = masked, or NULL; cond_auto_threshold > 0 adds the
    // automatic mask) and, with cond_zero_dm, freed of its per-(time, beam) mean over the channels -- in the stage's buffer, so the
    // detected sinks keep the raw stream.  On a sharded run every rank that dedisperses conditions its gathered rows itself:
    // redundant and identical, nothing is exchanged.
    int cond_baseline = 0;
    bool cond_zero_dm = true;
    double cond_auto_threshold = 0.0;
    const uint8_t* cond_mask = nullptr;
    // Pulsar folding behind the DM stage (docs/PULSAR_FOLDING.md; needs dm_delays): n_psr = 1 .. 4 pulsars (0 = off) with their
    // oscillators psr_models [n_psr] (bf_psr_model_from_spin) and delays psr_delays (host int32 [n_psr][cfg.n_freq * world], >= 0, a row
    // of dm_delays each), psr_bins phase bins.  A bf_psr is created next to the DM stage and attached to it: it folds every pushed block
    // where it lies in the stage's buffer (conditioned, if cond_baseline > 0).  After every launch that brings the rows folded since the
    // last dump to psr_dump_rows or more the folder is dumped; every dump goes to psr_sink once its block has been analysed (an incomplete
    // integration at the end is dropped).  On a sharded run the ranks that dedisperse each fold the whole band: redundant and identical.
    const bf_psr_model* psr_models = nullptr;
    const int32_t* psr_delays = nullptr;
    int n_psr = 0;
    int psr_bins = 64;
    int psr_dump_rows = 0;
    dsabf::psr_sink* psr_sink = nullptr;
    // Pulse injection in front of the DM stage (docs/INJECTION.md; needs dm_delays): a plan of bursts and trains (NULL or empty = off) whose
    // tables span the whole band (cfg.n_freq * world channels) and cfg.n_beams beams.  A bf_inj of exactly the plan's size is created next to
    // the DM stage, every pulse is added before the first push (the bursts' ids first), and it is attached: the pulses are added to every
    // pushed block where it lies in the stage's buffer, in front of the conditioner; the detected sinks keep the raw stream.  On a sharded
    // run every rank that dedisperses injects the whole band: redundant and identical, as the folder folds.
    const dsabf::inj_plan* inj = nullptr;
    // Periodicity search behind the DM stage (docs/PERIODICITY.md; needs dm_delays): ffa_p_hi > 0 switches it on.  The chunks of this
    // rank's trials are decimated by ffa_dec and cut into segments of ffa_seg samples; every segment is folded at the base periods
    // ffa_p_lo <= p < ffa_p_hi of ffa_oct octaves with ffa_widths boxcar widths (the bounds of bf_ffa_create).  The stage is created
    // next to the DM stage with dm_first from the plan and attached; every segment's candidates at or above ffa_threshold go to
    // ffa_sink (may be NULL: the stage still runs).  A segment that is incomplete when the run ends is dropped.
    int ffa_p_lo = 0, ffa_p_hi = 0;
    int ffa_seg = 1024, ffa_dec = 1, ffa_oct = 1, ffa_widths = 3;
    double ffa_threshold = 8.0;
    int ffa_detrend_blk = 0, ffa_detrend_win = 0;   // bf_ffa_set_detrend, applied right after the stage is created (0: off)
    dsabf::ffa_sink* ffa_sink = nullptr;
    // The incoherent beam (docs/INCOHERENT_BEAM.md): beam column `incoherent_beam` of the detected stream carries the antenna powers
    // summed over the antennas instead of a tied beam (bf_set_incoherent_beam, set on the handle before the loop); -1 = off.  On a
    // sharded run every rank gives the same index: the sum is per channel, each shard fills its own slice of the column.
    int incoherent_beam = -1;
    // The correlator (docs/CORRELATOR.md; needs block_launch): corr_blocks = analysed blocks integrated per dump, 0 = off.  Every dump
    // goes to vis_sink (may be NULL: the stage still runs).  An integration that is incomplete when the run ends is dropped.  On a
    // sharded run every rank correlates its own channels and has a sink of its own; the gather is untouched.
    int corr_blocks = 0;
    dsabf::vis_sink* vis_sink = nullptr;
    // The voltage moments (docs/SPECTRAL_KURTOSIS.md; needs block_launch): sk_blocks = analysed blocks integrated per dump, 0 = off.
    // Every dump goes to sk_sink (may be NULL: the stage still runs); an incomplete integration at the end of the run is dropped.  On a
    // sharded run every rank measures its own channels and has a sink of its own.
    int sk_blocks = 0;
    dsabf::sk_sink* sk_sink = nullptr;
    // -A: one layer of gains for THIS rank's channels, host [freq][ant]{re, im}: as debug_run_options::gains.
    const double* gains = nullptr;
    const uint8_t* ant_flags = nullptr;   // -f with -A: uint8 [n_ant], flagged antennas get zero weights (needs gains)
    const null_vectors* nulls = nullptr;  // -Z: as debug_run_options::nulls, for THIS rank's channels; the Stokes stage gets the same weights
    // Full-Stokes follow-up beams (docs/STOKES.md; needs block_launch): the beams to follow (empty = off; 1 .. 16 distinct indices), the
    // integration window in samples (0 = n_avg; must divide n_out_per_gemm * n_avg) and where every launch's set goes (may be NULL: the
    // stage still runs).  The stage holds (MAX_TOTAL_SEP + 2) x launches-per-block result sets of a block's entries each, on the device and
    // pinned: the run logs that amount and is refused (BF_ERR_INVALID, nothing allocated) beyond 8 GiB per side.  On a sharded run every rank follows the beams in its own channels and has a sink of its own.
    std::vector<int> stokes_beams;
    int stokes_int = 0;
    dsabf::stokes_sink* stokes_sink = nullptr;
};
struct observation_result {
    float observation_time_ms = 0;
    uint64_t blocks = 0;            // blocks analysed
    uint64_t data_chunks = 0;       // blocks * N_GEMMS_PER_BLOCK * N_OUTPUTS_PER_GEMM
    double gbytes_per_s = 0;        // "Approximate datarate", src/beamformer.cu:554
    std::vector<float> beam_out;    // final contents of beam_out: [stream][N_F_PER_DETECT] (src/beamformer.cu:249,485-488)
    std::vector<long long> last_gemm;  // global gemm-unit index (block * N_GEMMS_PER_BLOCK + time_slice) behind each stream
    uint64_t dm_times = 0;          // output times the DM stage produced (dm_delays set): rows analysed - the largest delay
    uint64_t dm_chunks = 0;         // chunks handed to dm_sink
    uint64_t sps_candidates = 0;    // candidates the search stage found (sps_widths > 0)
    uint64_t events = 0;            // events the builder closed (evt set), the final flush included
    uint64_t stamps = 0;            // stamps cut and handed to stamp_sink
    uint64_t stamps_dropped = 0;    // events beyond stamp_max_per_deliver of their deliver
    uint64_t stamps_missed = 0;     // requests whose rows had left the ring (status 1)
    uint64_t stamps_beyond_end = 0; // requests whose window passes the last row of the run: still "not pushed yet" at the last cut
    uint64_t vcuts = 0;             // voltage cuts handed to vcut_sink
    uint64_t vcuts_dropped = 0;     // events beyond vcut_max_per_deliver of their feed
    uint64_t vcuts_missed = 0;      // requests whose units had left the voltage history (status 1)
    uint64_t vcuts_beyond_end = 0;  // requests whose window passes the last unit of the run: still "not pushed yet" at the last cut
    uint64_t vis_dumps = 0;         // integrations the correlator dumped (corr_blocks > 0)
    uint64_t sk_dumps = 0;          // integrations the moments stage dumped (sk_blocks > 0)
    uint64_t stokes_units = 0;      // gemm-units the Stokes stage delivered (stokes_beams non-empty)
    uint64_t psr_dumps = 0;         // integrations the pulsar folder dumped (n_psr > 0)
    uint64_t inj_pulses = 0;        // pulses the injector was given (inj set and not empty)
    uint64_t ffa_segments = 0;      // segments the periodicity search collected (ffa_p_hi > 0)
    uint64_t ffa_candidates = 0;    // ... and the candidates they gave
    int cond_masked = -1;           // channels the conditioner masked in the last push (cond_baseline > 0 and a block analysed), else -1
};
// The reference's production main() loop on top of the C-ABI.  pos/dir: antenna positions and beam directions.
int run_observation(const bf_config& cfg, const observation_options& opt, block_source& source, const antenna* pos,
                    const beam_direction* dir, observation_result* res, std::ostream& log);

}  // namespace dsabf
