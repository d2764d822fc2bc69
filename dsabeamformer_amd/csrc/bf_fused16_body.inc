// bf_fused16_body.inc -- the text of fused16_kernel, fused16_fold_kernel and fused16_fold_stream_kernel (bf_fused16.hpp), included into
// all three.  In scope where it is included: the kernel argument `FusedArgs a` and the compile-time parameters AIN, NIPO, WRITE_C, MODE,
// PAIRED, WAVES, NS, FOLD, STREAM.
    constexpr int THREADS = 64 * WAVES;
    constexpr bool FAST = MODE == kDetFast;
    constexpr bool CONTRACTED = MODE == kDetContracted;
    // NIPO = 0: the accumulation window is a RUN-TIME value (any n_pol * n_avg that is not one of the compile-time windows; round 4).
    // A lane group's 32 rows of a chunk are then rt_kout whole windows back to back (or one window over rt_cpg chunks), padded
    // to 32 rows -- the stream scheme of fusedg_kernel in this kernel's weight-stationary loop; window starts and ends are
    // wave-uniform run-time flags per row.
    constexpr bool RTW = NIPO == 0;
    constexpr int MAPN = RTW ? 32 : NIPO;                // row <-> stream mapping and LDS swizzle: as for windows >= 32
    static_assert(!FAST || ((NIPO >= 16 || RTW) && !WRITE_C), "the fast detect exists for n_ipo >= 16 only");
    static_assert(!RTW || (WAVES == kWaves16 && NS == kColTiles16 && !ant_deep<AIN>()), "run-time windows: the plain launch shape");
    static_assert(!(PAIRED && WRITE_C), "the stage-parity path always runs the general kernel");
    static_assert(AIN >= kAntK3P4 && AIN != 0 && (AIN < 0 || AIN % 4 == 0) && AIN <= 256, "antenna class");
    static_assert(!ant_deep<AIN>() || (WAVES == 8 && NIPO >= 16 && !WRITE_C), "deep classes: 8 waves, long windows");
    static_assert(!FOLD || (AIN == kAntK1P16 && NIPO >= 16 && !WRITE_C && !PAIRED && WAVES == kWaves16 && NS == kColTiles16),
                  "antenna fold: 64 antennas in 16-byte pieces, long compile-time windows, general tiles on the plain launch shape");
    static_assert(!STREAM || FOLD, "the streamed chunk loop exists for the antenna-fold kernels");
    // the deep classes' operands count in units of the nibble value itself, not 16 x, staged as OFFSET nibbles v + 8 in [0, 15] with
    // the correction in the accumulator seeds (sign-extended nibbles cost 9 VALU per dword and the pipe holds a lower clock on them:
    // profiles/r04_ubench_encoding.txt)
    constexpr bool OFFSET_NIB = ant_deep<AIN>();
    constexpr float kA = FOLD ? kAlpha8 : OFFSET_NIB ? kAlpha : kAlpha16;   // accumulator unit -> alpha
    constexpr float kNKA = FOLD ? kNegMagicAlpha8 : OFFSET_NIB ? kNegMagicAlpha : kNegMagicAlpha16;
    constexpr bool RT = AIN < 0;                         // antenna count known only at run time
    constexpr int RB = 128;
    constexpr int KS = ant_ksteps<AIN>();                // k-steps of 64 antennas
    constexpr int PLANE = kRowsPerChunk * RB;            // LDS bytes of one k-step's chunk image
    constexpr int BUF = KS * PLANE;
    constexpr bool DW = RT ? (AIN == kAntK1P4 || AIN == kAntK2P4 || AIN == kAntK3P4 || AIN == kAntK4P4) : (AIN % 16) != 0;  // rows only dword-aligned: 4-byte pieces
    constexpr int PB = DW ? 4 : 16;                      // bytes per staging piece
    constexpr int AMAX = RT ? 64 * KS : AIN;             // most antennas this instantiation can meet
    const int A = FOLD ? 64 : RT ? a.n_ant : AIN;        // antennas per time sample (constant-folded unless RT)
    const int PPR = A / PB;                              // pieces per time sample
    const int TOTALP = kRowsPerChunk * PPR;              // pieces per chunk
    constexpr int TOTALP_MAX = kRowsPerChunk * (AMAX / PB);
    constexpr int NT = PAIRED ? NS / 2 : NS;             // MFMA column tiles per wave (a paired tile feeds 2 slots)
    constexpr bool LONG = NIPO >= 16;
    constexpr int L = LONG ? NIPO : 16;                  // samples per stream
    constexpr int LR = (NIPO >= 32 || RTW) ? 32 : 16;    // stream rows held by one chunk
    constexpr int CPG = L > 32 ? L / 32 : 1;             // chunks per group of 4 streams
    constexpr int PPT = (TOTALP_MAX + THREADS - 1) / THREADS;  // pieces per thread per chunk (2; 4; 13 for 100 antennas)
    using stage_t = std::conditional_t<DW, int, v4i>;

    extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 buffers x KS planes x 128 rows x 128 B

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g4 = lane >> 4;   // lane group = stream within the tile / k-block of the operands
    const int c16 = lane & 15;  // column within a 16-beam tile / A row

    int f, bg, ts;
    decode_block(a, f, bg, ts);
    const int cpg_rt = RTW ? a.rt_cpg : CPG;            // (constant-folded unless the window is a run-time value)
    const int units_total = a.chunks_total / cpg_rt;
    const int c_begin = (int)(((long long)units_total * ts) / a.n_tsplit) * cpg_rt;
    const int c_end = (int)(((long long)units_total * (ts + 1)) / a.n_tsplit) * cpg_rt;

    // ---- which beams this lane produces, and the weight fragments ------------------------------------------
    int slot_beam[NS];                                    // beam index of output slot s (>= n_beams: none)
    constexpr int NPC = kPairComps;                       // paired fragments per tile: Wr, Wi
    constexpr int NGC = FOLD ? kFoldComps : kGeneralComps;   // general fragments per tile: Wr, -Wi, Wi (the im row's Wr IS comp 0); FOLD: re row, im row
    v4i bw[NT][PAIRED ? NPC : NGC][KS];                   // general: [ct][Wr, -Wi, Wi][k-step]; paired: [pct][Wr, Wi][k-step]
    bool wave_active;
    if constexpr (PAIRED) {
        const int n_pct = a.n_ptiles;                     // pair tiles of 16 base beams = n_beams / 32
        const int pct0 = (bg * WAVES + wave) * NT;
        wave_active = pct0 < n_pct;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int bb = beam_of_tile(a.interleave ? NT : 0, pct0 + t, c16);  // base beam (< n_beams / 2)
            const bool ok = pct0 + t < n_pct;
            slot_beam[2 * t] = ok ? bb : a.n_beams;
            slot_beam[2 * t + 1] = ok ? a.n_beams - 1 - bb : a.n_beams;
#pragma unroll
            for (int comp = 0; comp < NPC; comp++)
#pragma unroll
                for (int h = 0; h < KS; h++)
                    bw[t][comp][h] =
                        ok ? a.wimg[((((size_t)f * n_pct + pct0 + t) * NPC + comp) * KS + h) * 64 + lane] : v4i{0, 0, 0, 0};
        }
    } else {
        const int n_ctiles = a.n_ctiles;
        const int ct0 = (bg * WAVES + wave) * NT;      // first 16-beam column tile of this wave
        wave_active = ct0 < n_ctiles;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const bool ok = ct0 + t < n_ctiles;
            slot_beam[t] = ok ? beam_of_tile(a.interleave ? NT : 0, ct0 + t, c16) : a.n_beams;
#pragma unroll
            for (int k = 0; k < NGC; k++)
#pragma unroll
                for (int h = 0; h < KS; h++)
                    bw[t][k][h] =
                        ok ? a.wimg[((((size_t)f * n_ctiles + ct0 + t) * NGC + k) * KS + h) * 64 + lane] : v4i{0, 0, 0, 0};
        }
    }

    v4i kc = {(int)kMagicBits, (int)kMagicBits, (int)kMagicBits, (int)kMagicBits};
    asm volatile("" : "+v"(kc));
    const v4i kzero = {0, 0, 0, 0};
    // Offset nibbles: sum W (v + 8) = sum W v + 8 sum W, so the chains start at seed - 8 * (this lane's column sum of the weight
    // fragment they multiply): summed here from the B fragments themselves (16 antennas per lane and k-step, the four lane groups
    // hold the other 48), once per workgroup.  General: sd[t][0] -> re = Wr Vr - Wi Vi, sd[t][1] -> im = Wi Vr + Wr Vi;
    // paired: sd[t][0] -> P1, P3 (Wr), sd[t][1] -> P2, P4 (Wi, no magic).
    [[maybe_unused]] v4i sd[OFFSET_NIB ? NT : 1][2];
    if constexpr (OFFSET_NIB) {
        auto colsum = [&](const v4i (&w)[KS]) {
            int sacc = 0;
#pragma unroll
            for (int h = 0; h < KS; h++)
#pragma unroll
                for (int d = 0; d < 4; d++)
#pragma unroll
                    for (int b = 0; b < 4; b++) sacc += (int)(signed char)((unsigned)w[h][d] >> (8 * b));
            sacc += __shfl_xor(sacc, 16);
            sacc += __shfl_xor(sacc, 32);
            return sacc;
        };
#pragma unroll
        for (int t = 0; t < NT; t++) {
            int s0, s1;
            if constexpr (PAIRED) {
                s0 = (int)kMagicBits - 8 * colsum(bw[t][0]);
                s1 = -8 * colsum(bw[t][1]);
            } else {
                const int wr = colsum(bw[t][0]), nwi = colsum(bw[t][1]), wi = colsum(bw[t][2]);
                s0 = (int)kMagicBits - 8 * (wr + nwi);
                s1 = (int)kMagicBits - 8 * (wi + wr);
            }
            sd[t][0] = v4i{s0, s0, s0, s0};
            sd[t][1] = v4i{s1, s1, s1, s1};
            asm volatile("" : "+v"(sd[t][0]), "+v"(sd[t][1]));
        }
    }

    // ---- staging (the chunk's 128 samples are contiguous in time for n_ipo <= 32) ------------------------------
    auto run_sample0 = [&](int c, int run) -> unsigned {   // first global sample of stream-run `run` of chunk c
        if constexpr (RTW)
            return (4u * (unsigned)(c / cpg_rt) + (unsigned)run) * (unsigned)a.rt_Ls + 32u * (unsigned)(c % cpg_rt);
        else if constexpr (NIPO >= 32)
            return (4u * (unsigned)(c / CPG) + (unsigned)run) * (unsigned)L + 32u * (unsigned)(c % CPG);
        else
            return (unsigned)c * 128u + 16u * (unsigned)run;
    };
    stage_t stage[PPT];
    // Fast addressing: when a chunk's sample span (128 samples, 256 for n_ipo = 64) never straddles a gemm-unit, the
    // unit / time split of the chunk is wave-uniform -- a scalar base that advances by one span per chunk -- and the
    // per-lane part (row and piece) is a constant 32-bit offset: no vector integer arithmetic (the generic
    // path costs ~17 VALU ops, 6 of them quarter-rate 32-bit multiplies, per load).
    constexpr unsigned SPAN = (NIPO == 64) ? 256u : 128u;
    const bool fast_addr = !RTW && ((unsigned)a.T % SPAN) == 0;
    // Piece k of this thread is piece pc = tid + 256 k of the chunk: row pc / PPR, position pc % PPR.  Its byte offset
    // from the chunk's first sample is PB * pc (rows are PPR * PB bytes and consecutive) -- except for n_ipo = 64, whose
    // chunk rows are four runs of 32 samples, 64 apart.  The 16*im image sits 4 pieces away from the 16*re image (after it
    // in plane 0, before it in plane 1), and the swizzle only XORs the 3 piece bits, so its LDS offset is the re offset ^ 64.
    [[maybe_unused]] unsigned lane_off64[NIPO == 64 ? PPT : 1];
    int lds_re[PPT];                      // LDS byte offset (inside one buffer) of the piece's 16*re image
    // FOLD: the chunk row a thread stages.  STREAM deals the rows so that the 8 lanes of a ds_write_b128 group (thread pairs q = tid / 2
    // = 4 j ... 4 j + 3) hold rows that differ in bit 0 and in the LOW STREAM BIT (row / LR & 1) -- the two row bits that swz16 XORs
    // into piece bits 2 and 1 -- and not, like rows 4 j ... 4 j + 3, in bits 0 and 1, of which bit 1 lands on the piece bit P itself:
    // with P the 8 lanes then cover all eight 16-byte slots of the 128-byte bank window (no store conflict; the four stores of a
    // thread XOR constants into the slot).  Which thread stages a row changes nothing else: offsets formed once, same LDS image.
    [[maybe_unused]] const int fold_row = [&] {
        const int q = tid >> 1;
        if constexpr (!STREAM) return q;
        else if constexpr (LR == 32) return (q & 1) | (((q >> 1) & 3) << 5) | (((q >> 3) & 15) << 1);
        else return (q & 1) | (((q >> 1) & 3) << 4) | (((q >> 3) & 7) << 1) | ((q >> 6) << 6);
    }();
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        int row, pi;
        if constexpr (FOLD) {   // a thread takes piece P = tid & 1 of row tid / 2 (STREAM: fold_row; k = 0) and its mirror piece 3 - P (k = 1): antenna 16 P + j <-> byte 15 - j
            if constexpr (STREAM) row = fold_row;
            else row = tid >> 1;
            pi = k == 0 ? (tid & 1) : 3 - (tid & 1);
        } else {
            const int pc = tid + k * THREADS;
            row = (pc / PPR) % kRowsPerChunk, pi = pc % PPR;   // (% keeps the unused tail pieces in range)
        }
        if constexpr (NIPO == 64) lane_off64[k] = (unsigned)((row / LR) * L + (row % LR)) * A + pi * PB;
        const int blk = DW ? pi / 4 : pi;                            // 16-antenna block of the piece
        const int h = blk / 4, kp = blk % 4, sub = DW ? 4 * (pi % 4) : 0;
        lds_re[k] = h * PLANE + row * RB + 16 * swz16<MAPN>(kp + 4 * (h & 1), row) + sub;  // plane 1: halves swapped
    }
    auto lane_off = [&](int k) -> unsigned {
        if constexpr (NIPO == 64)
            return lane_off64[k];
        else if constexpr (STREAM)
            return (unsigned)(64 * fold_row + 16 * (k == 0 ? (tid & 1) : 3 - (tid & 1)));
        else if constexpr (FOLD)
            return (unsigned)(64 * (tid >> 1) + 16 * (k == 0 ? (tid & 1) : 3 - (tid & 1)));
        else
            return (unsigned)PB * (unsigned)(tid + k * THREADS);
    };
    auto piece_live = [&](int k) { return (!RT && TOTALP_MAX % THREADS == 0) || (tid + k * THREADS < TOTALP); };
    int ld_span = -1;                 // span the scalar state below describes
    unsigned ld_u = 0, ld_t0 = 0;     // its gemm-unit and first sample inside the unit
    auto load_chunk = [&](int c) {
        if (fast_addr) {
            const int span = (NIPO == 64) ? c / 2 : c;
            if (ld_span < 0) {
                const unsigned s_c = (unsigned)span * SPAN;
                ld_u = a.t_shift >= 0 ? (s_c >> a.t_shift) : (s_c / (unsigned)a.T);
                ld_t0 = s_c - ld_u * (unsigned)a.T;
                ld_span = span;
            }
            while (ld_span < span) {  // at most one step: chunks are loaded in order
                ld_t0 += SPAN;
                if (ld_t0 >= (unsigned)a.T) {
                    ld_t0 = 0;
                    ld_u++;
                }
                ld_span++;
            }
            const bool valid = (unsigned)span * SPAN < a.S;
            const unsigned half = (NIPO == 64) ? 32u * (unsigned)(c & 1) : 0u;
            const uint8_t* base = a.in + ((size_t)((size_t)ld_u * a.n_freq + f) * a.T + ld_t0 + half) * A;
#pragma unroll
            for (int k = 0; k < PPT; k++) {
                stage[k] = stage_t{};
                if (valid && piece_live(k)) stage[k] = *reinterpret_cast<const stage_t*>(base + lane_off(k));   // (nontemporal: +-0.5 %, r02_variants_log)
            }
            return;
        }
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            int row, pi;
            if constexpr (FOLD) {
                row = tid >> 1;
                pi = k == 0 ? (tid & 1) : 3 - (tid & 1);
            } else {
                const int pc = tid + k * THREADS;       // (run-time antenna classes: a real division per piece, but this is
                row = (pc / PPR) % kRowsPerChunk, pi = pc % PPR;   //  the path of small DEBUG-style gemm-units only)
            }
            const unsigned s0 = run_sample0(c, row / LR) + (unsigned)(row % LR);
            stage[k] = stage_t{};
            bool row_ok = s0 < a.S;
            if constexpr (RTW) row_ok = row_ok && 32u * (unsigned)(c % cpg_rt) + (unsigned)(row % LR) < (unsigned)a.rt_Ls;   // not a padding row
            if (row_ok && piece_live(k)) {
                const unsigned u = a.t_shift >= 0 ? (s0 >> a.t_shift) : (s0 / (unsigned)a.T);
                const unsigned t = s0 - u * (unsigned)a.T;
                stage[k] = *reinterpret_cast<const stage_t*>(a.in + ((size_t)((size_t)u * a.n_freq + f) * a.T + t) * A + pi * PB);
            }
        }
    };
    // STREAM (fused16_fold_stream_kernel; launched only when T % SPAN == 0, launch_fused16_fold_stream_t): the chunk addressing above
    // as wave-uniform state that advances by a constant, and a prefetch with no predicate.
    //  * Every chunk of [0, chunks_total) holds real samples only: T % SPAN == 0 makes S = n_units * T a multiple of SPAN, hence of
    //    4 * n_ipo (SPAN = 128 for n_ipo 16 / 32, 256 for 64), so fused_launch_shape's rows = ceil(S / n_ipo / 4) * 4 * n_ipo == S and
    //    chunks_total * 128 == S (the launcher refuses anything else).  `valid` is constant-true; so is piece_live (256 threads x 2
    //    pieces = the chunk's 512 pieces).  No zero-initialisation, no branch around a load.
    //  * st_base = first byte of chunk st_next, the chunk the next load_stream() requests: 64-bit and scalar (a launch may exceed
    //    4 GiB); the per-lane part is lane_off(k), 32-bit and constant for the whole kernel.  One chunk on = 128 samples (n_ipo 64:
    //    32 samples inside a span, 224 to the next span); a span that would start at sample T starts the next gemm-unit instead, which
    //    lies (n_freq - 1) * T samples further on.
    //  * The requests are clamped to the workgroup's last chunk: the last two requests of a workgroup re-read chunk c_end - 1 (real
    //    samples, see above) and nobody reads what is staged from them.
    [[maybe_unused]] unsigned long long st_base = 0;   // (bytes behind a.in)
    [[maybe_unused]] unsigned st_t0 = 0;      // first sample of st_next's span inside its gemm-unit
    [[maybe_unused]] int st_next = c_begin;
    [[maybe_unused]] unsigned long long st_unit = 0;   // bytes from a gemm-unit's end to the same frequency's next gemm-unit
    [[maybe_unused]] unsigned st_off[PPT];             // lane_off(k), formed once
    // (64-bit products are formed on the vector unit, once per workgroup: the state goes back to scalar registers by name)
    [[maybe_unused]] auto sgpr64 = [](unsigned long long v) {
        return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v) |
               ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32);
    };
    if constexpr (STREAM) {
        const unsigned s_c = (unsigned)(NIPO == 64 ? c_begin / 2 : c_begin) * SPAN;   // (n_ipo 64: c_begin is even, a whole group)
        const unsigned u = a.t_shift >= 0 ? (s_c >> a.t_shift) : (s_c / (unsigned)a.T);
        st_t0 = s_c - u * (unsigned)a.T;
        st_base = sgpr64((unsigned long long)((size_t)((size_t)u * a.n_freq + f) * a.T + st_t0) * 64);
        st_t0 = (unsigned)__builtin_amdgcn_readfirstlane((int)st_t0);
        st_unit = sgpr64((unsigned long long)(unsigned)(a.n_freq - 1) * (unsigned)a.T * 64);
#pragma unroll
        for (int k = 0; k < PPT; k++) st_off[k] = lane_off(k);
    }
    // STREAM: what the chunk loop needs besides the samples, as per-lane registers formed once per workgroup (docs/LOG_r09.md).
    //  * fk: the staging's masks and the byte-reversal selector (bf_fold_staging.h) -- operands, not 32-bit literals behind the opcode.
    //  * wr_ptr / rd_ptr: the LDS addresses of the four staging stores (sr, di, dr, si) and of the two fragment reads of row tile 0,
    //    INCLUDING the buffer -- no scalar buffer base added to a per-lane constant in front of every store and read.  Both start in
    //    buffer 0.  wr_ptr moves by lds_step behind every staging (+BUF, -BUF, ...: the prologue stages into buffer 0, the first
    //    chunk into buffer 1); rd_ptr moves the other way behind every chunk of the tile loop, towards the buffer that chunk's
    //    staging filled; lds_step changes sign once per staged chunk, as its last use there (a negation in place, no copy).
    //    Row tile t8 of a lane lies RB * lds_row16(t8, 0) bytes behind its row tile 0: the row splits into a t8 part and a lane
    //    part, and the swizzle reads only row bits of the lane part.
    using lds_ptr = __attribute__((address_space(3))) char*;
    using lds_v4i = __attribute__((address_space(3))) v4i;
    [[maybe_unused]] FoldStageMasks fk;
    [[maybe_unused]] lds_ptr wr_ptr[4] = {nullptr, nullptr, nullptr, nullptr}, rd_ptr[2] = {nullptr, nullptr};
    [[maybe_unused]] int lds_step = BUF;
    if constexpr (STREAM) {
        static_assert(KS == 1, "one plane per buffer");
        asm volatile("" : "+v"(fk.m78), "+v"(fk.kC0), "+v"(fk.k40), "+v"(fk.f0f), "+v"(fk.k18), "+v"(fk.k08), "+v"(fk.h80), "+v"(fk.f8), "+v"(fk.rev),
                     "+v"(lds_step));
#pragma unroll
        for (int j = 0; j < 4; j++) wr_ptr[j] = (lds_ptr)smem + (lds_re[0] ^ (32 * j));
        const int row0 = lds_row16<MAPN>(0, c16);
        rd_ptr[0] = (lds_ptr)smem + (row0 * RB + 16 * swz16<MAPN>(g4, row0));
        rd_ptr[1] = (lds_ptr)smem + (row0 * RB + 16 * swz16<MAPN>(g4 + 4, row0));
    }
    auto load_stream = [&]() {
        // (the base as a scalar register pair by name, the pointer global by type: global_load v, v_off, s[base] -- not a.in + lane_off
        //  hoisted into four VGPRs and a 64-bit vector add per load)
        unsigned long long base = (unsigned long long)a.in + st_base;
        asm volatile("" : "+s"(base));
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            // (its zero extension stays beside the load, where the instruction's 32-bit offset operand takes it; pinned in its own
            //  register, not in a copy: a copy is a v_mov per load and chunk)
            asm volatile("" : "+v"(st_off[k]));
            stage[k] = *(const __attribute__((address_space(1))) stage_t*)(base + st_off[k]);
        }
        if (st_next + 1 < c_end) {             // scalar: no memory operation depends on it
            bool next_span = true;
            if constexpr (NIPO == 64) {
                next_span = (st_next & 1) != 0;
                st_base += next_span ? (size_t)(SPAN - 32u) * 64 : (size_t)32 * 64;
            } else {
                st_base += (size_t)SPAN * 64;
            }
            if (next_span) {
                st_t0 += SPAN;
                if (st_t0 >= (unsigned)a.T) {
                    st_t0 = 0;
                    st_base += st_unit;
                }
            }
            st_next++;
        }
    };
    auto write_chunk = [&](char* buf) {
        if constexpr (FOLD) {
            // stage[0] = antennas 16 P ... 16 P + 15 of the row, stage[1] = their mirror images in descending order.  Per dword pair:
            // the mirror dword byte-reversed (v_perm_b32), offset nibbles t = w ^ 0x88 (n + 8 in [0, 15]), h = 8 (n + 8) in [0, 120] per
            // byte (re: bits 4-7, im: bits 0-3 of the packed byte), then per byte 8 S = (h_a + h_b) - 128 and 8 D = (h_a + 128 - h_b) - 128:
            // no carry, no borrow between the bytes, two's-complement int8 in [-128, 112] and [-120, 120].  An all-zero row
            // (behind the launch's last sample) gives all-zero operands.  LDS row: Sr0 Sr1 Di0 Di1 | Dr0 Dr1 Si0 Si1 (pieces
            // P, P + 2, P + 4, P + 6: the swizzle only XORs the 3 piece bits).
            constexpr unsigned M = 0x78787878u, H = 0x80808080u;
            v4i sr, si, dr, di;
            if constexpr (STREAM) {   // the chunk loop's one wait for global memory: both prefetched pieces at once, stated here so that
                __builtin_amdgcn_s_waitcnt(0x0F70);   // the compiler adds none of its own (vmcnt(0); expcnt and lgkmcnt left alone)
                asm volatile("" : "+v"(stage[0]), "+v"(stage[PPT - 1]));
                // the same bytes in 16 operations per dword pair (fold_stage_pair, bf_fold_staging.h), stored through wr_ptr; `buf` is
                // the buffer wr_ptr already points into
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    unsigned xsr, xsi, xdr, xdi;
                    fold_stage_pair((unsigned)stage[0][d], (unsigned)stage[PPT - 1][3 - d], fk, xsr, xsi, xdr, xdi);
                    sr[d] = (int)xsr, si[d] = (int)xsi, dr[d] = (int)xdr, di[d] = (int)xdi;
                }
                *reinterpret_cast<lds_v4i*>(wr_ptr[0]) = sr;
                *reinterpret_cast<lds_v4i*>(wr_ptr[1]) = di;
                *reinterpret_cast<lds_v4i*>(wr_ptr[2]) = dr;
                *reinterpret_cast<lds_v4i*>(wr_ptr[3]) = si;
#pragma unroll
                for (int j = 0; j < 4; j++) wr_ptr[j] += lds_step;
                return;
            }
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const unsigned ta = (unsigned)stage[0][d] ^ 0x88888888u;
                const unsigned tb = __builtin_bswap32((unsigned)stage[PPT - 1][3 - d]) ^ 0x88888888u;
                const unsigned ra = (ta >> 1) & M, ia = (ta << 3) & M, rb = (tb >> 1) & M, ib = (tb << 3) & M;
                sr[d] = (int)((ra + rb) ^ H);
                si[d] = (int)((ia + ib) ^ H);
                dr[d] = (int)(((ra | H) - rb) ^ H);
                di[d] = (int)(((ia | H) - ib) ^ H);
            }
            *reinterpret_cast<v4i*>(buf + lds_re[0]) = sr;
            *reinterpret_cast<v4i*>(buf + (lds_re[0] ^ 32)) = di;
            *reinterpret_cast<v4i*>(buf + (lds_re[0] ^ 64)) = dr;
            *reinterpret_cast<v4i*>(buf + (lds_re[0] ^ 96)) = si;
            return;
        }
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            if (!piece_live(k)) continue;
            if constexpr (DW) {
                const unsigned w = (unsigned)stage[k];
                if constexpr (OFFSET_NIB) {          // (the deep classes' encodings: see the 16-byte pieces below)
                    const unsigned x = w ^ 0x88888888u;
                    *reinterpret_cast<int*>(buf + lds_re[k]) = (int)((x >> 4) & 0x0F0F0F0Fu);
                    *reinterpret_cast<int*>(buf + (lds_re[k] ^ 64)) = (int)(x & 0x0F0F0F0Fu);
                } else {
                    *reinterpret_cast<int*>(buf + lds_re[k]) = (int)(w & 0xF0F0F0F0u);
                    *reinterpret_cast<int*>(buf + (lds_re[k] ^ 64)) = (int)((w << 4) & 0xF0F0F0F0u);
                }
            } else {
                v4i re, im;
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    const unsigned w = (unsigned)stage[k][d];
                    if constexpr (OFFSET_NIB) {   // v + 8 = the nibble's bits with the top one flipped
                        const unsigned x = w ^ 0x88888888u;
                        re[d] = (int)((x >> 4) & 0x0F0F0F0Fu);
                        im[d] = (int)(x & 0x0F0F0F0Fu);
                    } else {
                        re[d] = (int)(w & 0xF0F0F0F0u);
                        im[d] = (int)((w << 4) & 0xF0F0F0F0u);
                    }
                }
                *reinterpret_cast<v4i*>(buf + lds_re[k]) = re;
                *reinterpret_cast<v4i*>(buf + (lds_re[k] ^ 64)) = im;
            }
        }
    };

    const size_t FB = (size_t)a.n_freq * a.n_beams;
    float sum[NS];                         // running sum of this lane's current output, per slot
#pragma unroll
    for (int sl = 0; sl < NS; sl++) sum[sl] = 0.0f;
    constexpr int PEND = LONG ? (L >= 32 ? 1 : 2) : 1;   // outputs completed per chunk per lane (LONG)
    float pend[PEND][NS];
    int pend_chunk[PEND];                  // chunk whose finished sums sit in pend[gi] (-1: none); tracked per entry
#pragma unroll                             // because entry 0 of chunk c can be parked before entry 1 of chunk c-1 left
    for (int gi = 0; gi < PEND; gi++) pend_chunk[gi] = -1;
    // STREAM: entry gi of a workgroup parks the groups grp0, grp0 + step, ... in that order and every parked group is stored before the
    // next one is parked (flush_pending runs once per chunk), so the wave-uniform part of a store's address is scalar state like
    // st_base: st_ub[gi] = bytes from a.out to (row 4 * group, frequency f, beam 0) of the group entry gi stores next, advanced by one
    // add per store.  The per-lane part of an interleaved store, g4 * FB + the lane's first beam, is formed once (st_lane0, floats).
    [[maybe_unused]] unsigned long long st_ub[PEND], st_ub_step = 0;
    [[maybe_unused]] size_t st_lane0 = 0;
    if constexpr (STREAM) {
        constexpr unsigned GSTEP = (NIPO >= 32) ? 1u : 2u;   // groups between two stores of one entry
#pragma unroll
        for (int gi = 0; gi < PEND; gi++) {
            const unsigned grp0 = (NIPO >= 32) ? (unsigned)(c_begin / CPG) : (2u * (unsigned)c_begin + gi);
            st_ub[gi] = sgpr64((unsigned long long)((size_t)(4u * grp0) * FB + (size_t)f * a.n_beams) * sizeof(float));
        }
        st_ub_step = sgpr64((unsigned long long)(4u * GSTEP) * FB * sizeof(float));
        st_lane0 = (size_t)g4 * FB + (size_t)slot_beam[0];
    }
    // x[sl] -> row[beam of slot sl]; `row` points at beam 0 of one output's frequency row.  Interleaved tiles give every
    // lane consecutive beams: vector stores.
    auto store_slots = [&](float* row, const float (&x)[NS]) {
        if (a.interleave) {
            // Nontemporal: the powers are written once and read by nobody on this GPU before the D2H / gather.  Every
            // store instruction covers whole 128-byte lines (16 lanes x 16 B, or 16 x 8 B), so streaming them past L2
            // costs nothing at C3 / C5 (+0.3 %) and lifts the store-bound DEBUG geometry from 0.60 to 0.73 of 8 TB/s
            // (profiles/r02_variants_log.txt).  The scalar stores of non-interleaved tiles cover partial lines: plain.
            if constexpr (PAIRED && NS == 2) {   // one pair tile per wave (deep classes, beams not in groups of 512): beam bb and its mirror
                row[slot_beam[0]] = x[0];
                row[slot_beam[1]] = x[1];
            } else if constexpr (PAIRED && NS == 4) {   // slots 0, 2 = base beams bb, bb + 1; slots 1, 3 = their mirrors B-1-bb, B-2-bb
                __builtin_nontemporal_store(v2f{x[0], x[2]}, reinterpret_cast<v2f*>(row + slot_beam[0]));
                __builtin_nontemporal_store(v2f{x[3], x[1]}, reinterpret_cast<v2f*>(row + slot_beam[3]));
            } else if constexpr (PAIRED) {       // NS == 8: four base beams ascending, their four mirrors descending
                __builtin_nontemporal_store(v4f{x[0], x[2], x[4], x[6]}, reinterpret_cast<v4f*>(row + slot_beam[0]));
                __builtin_nontemporal_store(v4f{x[7], x[5], x[3], x[1]}, reinterpret_cast<v4f*>(row + slot_beam[7]));
            } else if constexpr (NS == 2) {       // two neighbouring beams per lane
                __builtin_nontemporal_store(v2f{x[0], x[1]}, reinterpret_cast<v2f*>(row + slot_beam[0]));
            } else {
#pragma unroll
                for (int q = 0; q < NS; q += 4)
                    __builtin_nontemporal_store(v4f{x[q], x[q + 1], x[q + 2], x[q + 3]}, reinterpret_cast<v4f*>(row + slot_beam[q]));
            }
        } else {
#pragma unroll
            for (int sl = 0; sl < NS; sl++)
                if (slot_beam[sl] < a.n_beams) row[slot_beam[sl]] = x[sl];
        }
    };
    auto flush_pending = [&]() {
        if constexpr (LONG && !WRITE_C) {
#pragma unroll
            for (int gi = 0; gi < PEND; gi++) {
                if constexpr (STREAM) {
                    // (chunks_total * 128 == S, so every output of every chunk lies inside the launch: see load_stream)
                    if (pend_chunk[gi] >= 0 && wave_active) {
                        float* ub = reinterpret_cast<float*>(reinterpret_cast<char*>(a.out) + st_ub[gi]);
                        if (a.interleave)   // (store_slots' vector store of four neighbouring beams: NS == 4, not PAIRED)
                            __builtin_nontemporal_store(v4f{pend[gi][0], pend[gi][1], pend[gi][2], pend[gi][3]}, reinterpret_cast<v4f*>(ub + st_lane0));
                        else
                            store_slots(ub + (size_t)g4 * FB, pend[gi]);
                        st_ub[gi] += st_ub_step;
                    }
                } else if (pend_chunk[gi] >= 0 && wave_active) {
                    const unsigned grp = (NIPO >= 32) ? (unsigned)(pend_chunk[gi] / CPG) : (2u * pend_chunk[gi] + gi);
                    float* ub = a.out + ((size_t)(4u * grp) * FB + (size_t)f * a.n_beams);  // wave-uniform part
                    const unsigned o = 4u * grp + (unsigned)g4;
                    if (o * (unsigned)L < a.S) store_slots(ub + (size_t)g4 * FB, pend[gi]);
                }
                pend_chunk[gi] = -1;
            }
        }
    };

    if (c_begin >= c_end) return;
#if DSABF_CLOCKPROBE
    const unsigned long long probe_t0 = __builtin_amdgcn_s_memtime(), probe_r0 = __builtin_amdgcn_s_memrealtime();
#endif

    if constexpr (STREAM) {
        load_stream();
        write_chunk(smem);
        load_stream();
    } else {
        load_chunk(c_begin);
        write_chunk(smem);
        if (c_begin + 1 < c_end) load_chunk(c_begin + 1);
    }
    __syncthreads();
    if constexpr (STREAM) lds_step = -lds_step;   // (behind every staged chunk, as the last use of the step: the next staging goes the other way)

    // FOLD: a wave without beams only stages; its chunks run in a loop of their own, so that the tile loop holds the (longer) staging once
    const bool stage_only = FOLD && !wave_active;
    if (stage_only)
        for (int c = c_begin; c < c_end; c++) {
            if constexpr (STREAM) {   // (the last iteration stages a second image of chunk c_end - 1 into the buffer nobody reads any more)
                write_chunk(smem + ((c - c_begin + 1) & 1) * BUF);
                load_stream();
            } else {
                if (c + 1 < c_end) write_chunk(smem + ((c - c_begin + 1) & 1) * BUF);
                if (c + 2 < c_end) load_chunk(c + 2);
            }
            __syncthreads();
            if constexpr (STREAM) lds_step = -lds_step;
        }
    for (int c = stage_only ? c_end : c_begin; c < c_end; c++) {
        [[maybe_unused]] char* cur = smem + ((c - c_begin) & 1) * BUF;   // (STREAM: rd_ptr / wr_ptr hold the buffers)
        [[maybe_unused]] char* nxt = smem + ((c - c_begin + 1) & 1) * BUF;
        if (!FOLD && !wave_active) {
            if (c + 1 < c_end) write_chunk(nxt);
            if (c + 2 < c_end) load_chunk(c + 2);
        } else {
            [[maybe_unused]] float ov[2][NS];   // n_ipo < 16: the outputs the current tile completed, per slot
            // run-time window (RTW): where the windows of this lane group's stream start and end in the current row tile, the
            // sums that ended there, and the stream-relative index of their outputs -- wave-uniform
            [[maybe_unused]] bool rt_st[4] = {false, false, false, false}, rt_en[4] = {false, false, false, false};
            [[maybe_unused]] unsigned rt_o[4] = {0, 0, 0, 0};
            [[maybe_unused]] float rt_x[4][NS];
            [[maybe_unused]] int rt_m = 0;            // position of the next row inside its window
            [[maybe_unused]] unsigned rt_oq = 0;      // windows of the stream that ended before the next row
            if constexpr (RTW) {
                const unsigned p0 = 32u * (unsigned)(c % cpg_rt);
                rt_m = (int)(p0 % (unsigned)a.rt_L);
                rt_oq = p0 / (unsigned)a.rt_L;
            }
            // detect + accumulate the 4 samples (fr, fi: accumulator bit patterns K + 16 n) of output slot sl
            auto detect = [&](const int t8, const v4f fr, const v4f fi, const int sl) {
                // stream position of this tile's rows and whether it starts / ends an output
                const int gi = (NIPO >= 32) ? 0 : (t8 >> 2);          // group inside the chunk (L = 16)
                const int q4 = (NIPO >= 32) ? (32 * (c % CPG) + 4 * t8) : 4 * (t8 & 3);  // position of register 0
                const unsigned grp = (NIPO >= 32) ? (unsigned)(c / CPG) : (2u * (unsigned)c + gi);
                const unsigned o = 4u * grp + (unsigned)g4;           // this lane's stream (output index if LONG)
                const int beam = slot_beam[sl];
                if constexpr (WRITE_C && RTW) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const unsigned pos = 32u * (unsigned)(c % cpg_rt) + 4u * t8 + r;
                        const unsigned sidx = (4u * (unsigned)(c / cpg_rt) + (unsigned)g4) * (unsigned)a.rt_Ls + pos;
                        if (pos < (unsigned)a.rt_Ls && sidx < a.S && beam < a.n_beams) {
                            v2f cv = {__builtin_fmaf(fr[r], kA, kNKA), __builtin_fmaf(fi[r], kA, kNKA)};
                            *reinterpret_cast<v2f*>(a.out + 2 * (((size_t)f * a.T + sidx) * a.n_beams + beam)) = cv;
                        }
                    }
                } else if constexpr (RTW) {
                    // run-time window: rt_st[r] / rt_en[r] say whether a window starts / ends at register r of this row tile
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        if constexpr (FAST) {
                            const float dr = fr[r] - kMagic, di = fi[r] - kMagic;
                            float sacc = rt_st[r] ? 0.0f : sum[sl];
                            sacc = __builtin_fmaf(dr, dr, sacc);
                            sum[sl] = __builtin_fmaf(di, di, sacc);
                            if (rt_en[r]) rt_x[r][sl] = sum[sl] * (kA * kA);
                        } else {
                            const float x = __builtin_fmaf(fr[r], kA, kNKA);
                            const float y = __builtin_fmaf(fi[r], kA, kNKA);
                            const float yy = y * y;
                            float pp;
                            if constexpr (CONTRACTED) {
                                pp = __builtin_fmaf(x, x, yy);
                            } else {
                                const float xx = x * x;
                                pp = xx + yy;
                            }
                            // (a window's first sample: 0 * sum + pp = pp, any other: 1 * sum + pp in ONE rounding = sum + pp -- the
                            //  select folded into the add; the sums are finite and >= +0)
                            sum[sl] = __builtin_fmaf(sum[sl], rt_st[r] ? 0.0f : 1.0f, pp);
                            if (rt_en[r]) rt_x[r][sl] = sum[sl];
                        }
                    }
                } else if constexpr (WRITE_C) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const unsigned sidx = o * (unsigned)L + (unsigned)(q4 + r);
                        if (o * (unsigned)L < a.S && beam < a.n_beams) {
                            v2f cv = {__builtin_fmaf(fr[r], kA, kNKA), __builtin_fmaf(fi[r], kA, kNKA)};
                            *reinterpret_cast<v2f*>(a.out + 2 * (((size_t)f * a.T + sidx) * a.n_beams + beam)) = cv;
                        }
                    }
                } else if constexpr (FAST) {
                    // BF_DETECT_FAST: d = 16 n exactly (one subtract), acc = fma(d, d, acc): 4 ops per sample;
                    // the (alpha/16)^2 scale is applied once per output when it is parked for the store.
                    float sacc = (q4 == 0) ? 0.0f : sum[sl];
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float dr = fr[r] - kMagic, di = fi[r] - kMagic;
                        sacc = __builtin_fmaf(dr, dr, sacc);
                        sacc = __builtin_fmaf(di, di, sacc);
                    }
                    asm volatile("" : "+v"(sacc));
                    sum[sl] = sacc;
                    if (q4 + 4 == L) {
                        pend[gi][sl] = sacc * (kA * kA);
                        pend_chunk[gi] = c;
                    }
                } else {
                    float p[4];
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float x = __builtin_fmaf(fr[r], kA, kNKA);
                        const float y = __builtin_fmaf(fi[r], kA, kNKA);
                        const float yy = y * y;
                        if constexpr (CONTRACTED) {
                            p[r] = __builtin_fmaf(x, x, yy);   // nvcc's reading of x*x + y*y (-fmad=true): mul, then fma
                        } else {
                            const float xx = x * x;
                            p[r] = xx + yy;
                        }
                    }
                    if constexpr (LONG) {
                        float sacc = (q4 == 0) ? p[0] : (sum[sl] + p[0]);
                        sacc = sacc + p[1];
                        sacc = sacc + p[2];
                        sacc = sacc + p[3];
                        asm volatile("" : "+v"(sacc));
                        sum[sl] = sacc;
                        if (q4 + 4 == L) {
                            pend[gi][sl] = sacc;
                            pend_chunk[gi] = c;
                        }
                    } else {
                        // 16-sample stream = 16/NIPO outputs; registers r hold positions q4 + r.  Finished outputs are
                        // collected per slot (ov) and stored together after the tile's last column tile.
                        if constexpr (NIPO == 2) {
                            ov[0][sl] = p[0] + p[1];
                            ov[1][sl] = p[2] + p[3];
                        } else if constexpr (NIPO == 4) {
                            float sacc = p[0] + p[1];
                            sacc = sacc + p[2];
                            ov[0][sl] = sacc + p[3];
                        } else {  // NIPO == 8
                            float sacc = (q4 % 8 == 0) ? p[0] : (sum[sl] + p[0]);
                            sacc = sacc + p[1];
                            sacc = sacc + p[2];
                            sacc = sacc + p[3];
                            asm volatile("" : "+v"(sacc));
                            sum[sl] = sacc;
                            ov[0][sl] = sacc;
                        }
                    }
                }
            };
            // stores of the outputs a short-window (n_ipo < 16) tile completed
            auto store_short = [&](const int t8) {
                if constexpr (!LONG && !WRITE_C && !RTW) {
                    const int gi = t8 >> 2, q4 = 4 * (t8 & 3);
                    const unsigned o = 4u * (2u * (unsigned)c + gi) + (unsigned)g4;   // this lane's 16-sample stream
                    if (o * 16u < a.S) {
                        float* base = a.out + ((size_t)o * (16 / NIPO)) * FB + (size_t)f * a.n_beams;
                        if constexpr (NIPO == 2) {
                            store_slots(base + (size_t)(q4 / 2) * FB, ov[0]);
                            store_slots(base + (size_t)(q4 / 2 + 1) * FB, ov[1]);
                        } else if constexpr (NIPO == 4) {
                            store_slots(base + (size_t)(q4 / 4) * FB, ov[0]);
                        } else {
                            if (q4 % 8 == 4) store_slots(base + (size_t)(q4 / 8) * FB, ov[0]);
                        }
                    }
                }
            };

            // LDS fragments of row-tile t8: a0[h] = 16*re, a1[h] = 16*im of 16 antennas x 16 samples per lane group, k-step h
            auto read_frag = [&](const int t8, v4i (&a0)[KS], v4i (&a1)[KS]) {
                if constexpr (STREAM) {   // (rd_ptr: the current buffer's row tile 0 of this lane; see its declaration)
                    a0[0] = *reinterpret_cast<const lds_v4i*>(rd_ptr[0] + RB * lds_row16<MAPN>(t8, 0));
                    a1[0] = *reinterpret_cast<const lds_v4i*>(rd_ptr[1] + RB * lds_row16<MAPN>(t8, 0));
                    return;
                }
                const int row = lds_row16<MAPN>(t8, c16);
#pragma unroll
                for (int h = 0; h < KS; h++) {  // plane 1 keeps (im | re): the two planes' staging writes then never collide
                    a0[h] = *reinterpret_cast<const v4i*>(cur + h * PLANE + row * RB + 16 * swz16<MAPN>(g4 + 4 * (h & 1), row));
                    a1[h] = *reinterpret_cast<const v4i*>(cur + h * PLANE + row * RB + 16 * swz16<MAPN>(g4 + 4 * ((h & 1) ^ 1), row));
                }
            };
            // acc = seed + sum over the k-steps of x[h] * w[h]  (one MFMA per k-step, chained through srcC)
            auto dot = [&](const v4i (&x)[KS], const v4i (&w)[KS], v4i acc) {
#pragma unroll
                for (int h = 0; h < KS; h++) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(x[h], w[h], acc, 0, 0, 0);
                return acc;
            };
            // One step = the MFMAs of column tile t on row-tile fragments (a0, a1); its SPS output slots land in
            // re[] / im[] as accumulator bit patterns K + 16 n.
            constexpr int SPS = PAIRED ? 2 : 1;                 // output slots per step
            auto issue = [&](const v4i (&a0)[KS], const v4i (&a1)[KS], const int t, v4i (&re)[SPS], v4i (&im)[SPS]) {
                const v4i k0 = OFFSET_NIB ? sd[OFFSET_NIB ? t : 0][0] : kc;                         // chain seeds (see sd above)
                const v4i k1 = OFFSET_NIB ? sd[OFFSET_NIB ? t : 0][1] : (PAIRED ? kzero : kc);
                if constexpr (PAIRED) {
                    const v4i p1 = dot(a0, bw[t][0], k0);     // Wr*Vr + K
                    const v4i p3 = dot(a1, bw[t][0], k0);     // Wr*Vi + K
                    const v4i p2 = dot(a1, bw[t][1], k1);     // Wi*Vi   (+-P2, +-P4 on the VALU: chaining them on the MFMA
                    const v4i p4 = dot(a0, bw[t][1], k1);     // Wi*Vr    pipe -- 5 or 6 MFMAs per pair tile -- lost, r03_ab_c3_pairmfma)
                    re[0] = p1 - p2;
                    re[1] = p1 + p2;
                    im[0] = p3 + p4;
                    im[1] = p3 - p4;
                } else if constexpr (FOLD) {
                    re[0] = dot(a0, bw[t][0], k0);            // (Sr | Di) x (Wr | -Wi)
                    im[0] = dot(a1, bw[t][NGC - 1], k1);      // (Dr | Si) x (Wi | Wr)
                } else {
                    re[0] = dot(a1, bw[t][1], dot(a0, bw[t][0], k0));              // Wr*Vr - Wi*Vi
                    im[0] = dot(a1, bw[t][0], dot(a0, bw[t][2], k1));              // Wi*Vr + Wr*Vi
                }
            };
            auto consume = [&](const int t8, const int t, const v4i (&re)[SPS], const v4i (&im)[SPS]) {
#pragma unroll
                for (int e = 0; e < SPS; e++) {  // paired: slot 2t = beam b, slot 2t+1 = beam B-1-b
                    detect(t8, __builtin_bit_cast(v4f, re[e]), __builtin_bit_cast(v4f, im[e]), SPS * t + e);
                }
            };
            // staging work in the shadow of the MFMA stream: the next chunk's LDS image after tile 1, the parked stores
            // of the previous chunk and the prefetch of chunk c+2 after tile 3
            // (STREAM: neither depends on c -- the one wait for the prefetched registers is write_chunk's first read of them, six row
            //  tiles after their request, and the request goes out before the parked stores, whose acknowledgement nothing waits for;
            //  the workgroup's last iteration stages a second image of its last chunk into the buffer nobody reads any more)
            auto staging = [&](const int t8) {
                if constexpr (STREAM) {
                    if (t8 == 1) write_chunk(nxt);
                    if (t8 == 3) {
                        load_stream();
                        flush_pending();
                    }
                } else {
                    if (t8 == 1 && c + 1 < c_end) write_chunk(nxt);
                    if (t8 == 3) {
                        flush_pending();
                        if (c + 2 < c_end) load_chunk(c + 2);
                    }
                }
            };
            // STREAM: row tile t8 + 1's fragments are requested behind the last MFMA of tile t8 and in front of that MFMA's detect (nothing
            // crosses the scheduling barrier), into registers of their own; tile t8 + 1 opens with ONE stated wait for both of them, so
            // the compiler adds none between its MFMAs.  121 - 124 registers (docs/LOG_r09.md section 3; requesting them behind ALL of a
            // tile's MFMAs, issued before any detect, takes 128 and scratch).
            [[maybe_unused]] v4i pf0[KS], pf1[KS];
            if constexpr (STREAM) read_frag(0, pf0, pf1);
#pragma unroll
            for (int t8 = 0; t8 < 8; t8++) {   // (requesting tile t8+1's LDS fragments one tile early was tried: pair kernel
                v4i a0[KS], a1[KS];            //  -2 % (129 VGPRs: 3 instead of 4 waves per SIMD), general +-0, r02 variants log;
                if constexpr (STREAM) {        //  deep classes, requested and pinned one tile early: +-0.5 %, r04 variants log)
                    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0); vmcnt and expcnt left alone
                    a0[0] = pf0[0], a1[0] = pf1[0];
                    asm volatile("" : "+v"(a0[0]), "+v"(a1[0]));
#pragma unroll
                    for (int t = 0; t < NT; t++) {
                        v4i re[SPS], im[SPS];
                        issue(a0, a1, t, re, im);
                        if (t == NT - 1 && t8 + 1 < 8) {
                            read_frag(t8 + 1, pf0, pf1);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        consume(t8, t, re, im);
                    }
                    staging(t8);
                    continue;
                }
                read_frag(t8, a0, a1);
                if constexpr (RTW) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        rt_st[r] = rt_m == 0;
                        rt_en[r] = ++rt_m == a.rt_L;
                        if (rt_en[r]) {
                            rt_m = 0;
                            rt_o[r] = rt_oq++;
                            rt_en[r] = rt_o[r] < (unsigned)a.rt_kout;   // (a "window" of padding rows behind the stream's last one is nobody's)
                        }
                    }
                }
#pragma unroll
                for (int t = 0; t < NT; t++) {   // (the compiler issues the first MFMAs of all chains before the dependent
                    v4i re[SPS], im[SPS];        //  second ones by itself; forcing that order changed nothing, r02 variants log)
                    issue(a0, a1, t, re, im);
                    consume(t8, t, re, im);
                }
                if constexpr (RTW && !WRITE_C) {   // the windows that ended in this row tile: their sums leave at once
                    const unsigned sigma = 4u * (unsigned)(c / cpg_rt) + (unsigned)g4;      // this lane's stream
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (rt_en[r]) {
                            const unsigned o = sigma * (unsigned)a.rt_kout + rt_o[r];
                            if ((unsigned long long)o * (unsigned)a.rt_L < a.S) store_slots(a.out + (size_t)o * FB + (size_t)f * a.n_beams, rt_x[r]);
                        }
                }
                store_short(t8);
                staging(t8);
            }
            if constexpr (STREAM) {   // (towards the buffer the staging of this chunk has just filled)
                rd_ptr[0] -= lds_step;
                rd_ptr[1] -= lds_step;
                asm volatile("" : "+v"(lds_step), "+v"(rd_ptr[0]), "+v"(rd_ptr[1]));   // (negate behind its last use, in its own register)
                lds_step = -lds_step;
            }
        }
        __syncthreads();
    }
    flush_pending();
#if DSABF_CLOCKPROBE
    __syncthreads();
    if (tid == 0) {
        const unsigned long long dt = __builtin_amdgcn_s_memtime() - probe_t0, dr = __builtin_amdgcn_s_memrealtime() - probe_r0;
        a.out[blockIdx.x] = (float)((double)dt / (double)dr * 0.1);  // s_memrealtime ticks at 100 MHz
    }
#endif
