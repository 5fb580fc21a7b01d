// ekf_device.h -- HBM data layout shared by the kernels and the host ABI of libekfslam_hip.so.
//
// One handle = B independent filters.  For filter b, every element of the (3+2N)^2 covariance has
// exactly ONE authoritative home (DESIGN.md "Data layout"):
//   rows/cols 0..2 (robot)            -> R  [b][3][xs]      kept current by the chain kernel
//   the 2x2 block of landmark l       -> D  [b][3][dn]      (xx, xy, yy) kept current by the chain kernel
//   every other P_LL entry (i' <= j') -> Bm [buf][b][tiles] 64x64 tiles of the upper triangle,
//                                                           MFMA-fragment-major inside a tile,
//                                                           written ONLY by the dense pass (k_flush)
// P_LL indices are "landmark space": i' = i - 3.
//
// Everything the chain kernel decides that changes P_LL is recorded as a rank-2 "slot"
//       P_LL(i', j') += sum_{e<2} FA[i'][e] * FB[j'][e]          (i' <= j', different landmarks)
// Two consecutive slots share one row of FA/FB [b][set][pair][row i'][4] (slot 2p in [0..1], slot 2p+1 in
// [2..3]): 16 rows x 4 = one 512-byte A (or B) operand of v_mfma_f64_16x16x4_f64, i.e. k = 4 carries two
// measurements, and one landmark's two rows = one 64-byte line.  An Old-landmark update (Update.cpp:188,
// 193-194) is the slot FA = -T, FB = K with T = K S; a New landmark (Update.cpp:169-177) is the slot
// FA = P_xL, FB = unit rows at the new landmark.  The dense pass applies a whole set of slots in one read and
// one write of Bm; with two slot sets (and, in overlap mode, two Bm buffers) the chain kernels of the next
// window run while the dense pass of this window streams through HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/ekfslam_c.h"

#define EKF_INF 999999999999.0 /* kalmanfilter.h:17 */
#define EKF_MAX_PENDING 32
#define EKF_MAX_PAIRS (EKF_MAX_PENDING / 2)
// An entry of ekf_update_polar on its way to the device (MatchScratch::ids of that call): the landmark in the low bits, the kind
// (EKF_POLAR_*) above them -- a landmark number stays below EKF_MAX_CAPACITY = 16 000 < 2^14.  A skipped entry stays -1.
#define POLAR_KIND_SHIFT 14
#define POLAR_ID_MASK ((1 << POLAR_KIND_SHIFT) - 1)
static_assert(EKF_MAX_CAPACITY <= (1 << POLAR_KIND_SHIFT), "a landmark number must fit below the kind");
#define EKF_CHAIN_MAX_THREADS 256 /* one control wave + up to 192 workers: one wave per SIMD, 512-VGPR budget */
#define EKF_CHAIN_MAX_WGS 64 /* workgroups sharing one filter in k_chain: one lane of a wave polls each */
#define EKF_CHAIN_MAX_OPS 64 /* operations per k_chain launch */
// one workgroup's record of a cross-workgroup arg-min exchange.  Every value is two 8-byte granules
// {32 payload bits, 32-bit tag}: winner data = values [0,16), the winner's rows of every slot = values
// of both open windows [16, 16 + 8*2*maxp), head {d, landmark} = values EKF_REC_HEAD, EKF_REC_HEAD + 1; padded to whole 128-byte lines
#define EKF_REC_HEAD (16 + 8 * 2 * EKF_MAX_PENDING)
#define EKF_REC_DOUBLES (2 * EKF_REC_HEAD + 16)

// op records: 8 doubles per (op, filter); r[7] is the type
enum { OP_NOP = 0, OP_PROP = 1, OP_MEAS = 2, OP_COMPASS = 3, OP_TRUTH = 4, OP_SKIP_SLOT = 5,
       OP_SCRIPT = 6 };  // (streamed commands only) run operations [r[1], r[1] + r[2]) of the record array whose device address is the bit pattern of r[0]: a short scripted chunk
// header decisions (internal)
enum { HDR_NONE = 0, HDR_NEW = 1, HDR_OLD = 2, HDR_IGNORE = 3, HDR_COMPASS = 4, HDR_NEW_NOFIT = 5 };

// What kind of slot a measurement left behind, for the chain kernel's fold of the not-yet-flushed slots: an Old or
// compass slot contributes -K_i S K_j^T (S kept here), a New slot the column pair of landmark ln.
enum { SLOT_DEAD = 0, SLOT_OLD = 1, SLOT_NEW = 2 };
struct SlotMeta {
    int type, ln;
    double S00, S01, S11;
};

// What the host wants to see after every call (kalmanfilter.h:24-27 mirrors, sticky status, the newest
// gate decisions), written by k_chain into host-mapped pinned memory so that an API call needs no
// device-to-host copy: synchronise the stream, then read.
#define EKF_MIRROR_DECISIONS 64
struct EkfMirror {
    double pose[3];
    int n_lm;
    int status;
    long long log_count;
    long long seq;  // number of the chain launch that wrote this mirror last (stored last, system scope): the host may spin on it
    ekf_stats stats;  // the filter's counters as of that launch (ekf_get_stats without a device-to-host copy)
    double Prr[9];    // the robot block P[0:3,0:3], row-major (what kalmanfilter.cpp:51 logs a corner of: ekf_get_robot_cov without a copy)
    ekf_decision last[EKF_MIRROR_DECISIONS];  // entry i of the log lives at last[i % 64]
};

// One k_chain launch runs a list of segments; a segment is what used to be a launch of its own: a run of operations inside one
// slot set.  Several segments per launch keep the workgroups (their LDS caches, their registers) alive across window boundaries.
#ifndef EKF_PLAN_MAX
#define EKF_PLAN_MAX 12
#endif
struct ChainSeg {
    int k0, nops;        // operations [k0, k0 + nops) of the input
    int slot0;           // slots of the open set filled before this segment
    int set, buf_read;   // the open slot set; the P_LL buffer the segment reads
    int n_prev;          // slots of the other set still being folded by a dense pass (overlap mode)
    int need_pass;       // dense pass (number) that must have finished before this segment starts, 0 = none
    int drop;            // segments after the first: virtual slots that leave the LDS caches in front (the set whose pass has finished)
    long long seq;       // launch number (the host mirror shows the newest one that has finished)
    unsigned long long gate;  // multi-segment launches: the value dv.seg_count[this segment's index] shows when every workgroup has finished the segment
    int self_pass;       // k_solo: the segment fills its window and the workgroup folds it into its own P_LL tiles before it goes on (no dense-pass launch)
    int stagger;         // k_solo, first segment: filter b starts (b mod 4) * stagger ticks of the 100 MHz clock late (a phase shift between the
                         // filters of a batch, so that their own dense passes take turns in HBM); 0 = none
};
struct ChainPlan {
    int nseg;
    int signal;                     // != 0: every workgroup counts segment i in dv.seg_count[i] when it has finished it
    int inl_n;                      // != 0: the launch's one operation record (one filter, one operation: an immediate-mode call) travels in inl[]
                                    // with the kernel arguments instead of the host-mapped input ring: the kernel's first trip to host memory
                                    // (its arguments) brings the record along, where the ring costs a second, dependent one
    int stream;                     // != 0: a STREAMING launch (k_chain<true, true>, round 6), the value is its launch number: one segment with no
                                    // operations of its own; the operations arrive one by one through the command ring (StreamCtl, EkfDev::sring),
                                    // s[0].seq is the number of the last command consumed BEFORE this launch
    ChainSeg s[EKF_PLAN_MAX];
    double inl[8];
};

// ---- streaming immediate-mode calls (round 6) -----------------------------------------------------------------------------------
// The reference drives the filter one synchronising call per operation (slam.cpp:136-170).  As one kernel launch per call that is
// ~20 us per call around 1-7 us of device work: launch, dispatch, the workgroups' state reload (landmark registers, the own-row cache
// of the open window), completion.  A streaming launch stays resident instead: workgroup 0's control lane polls a command ring (in
// device memory the host writes through the BAR, or in host-mapped memory: EkfDev::sring), forwards each command to the filter's other workgroups through device memory, the operation runs exactly as
// it does inside a scripted segment, and workgroup 0 publishes the host mirror (pose, robot block, counts, decisions, sequence
// number) after EVERY operation.  The kernel leaves when the host says so (the window is full: the dense pass must run; any API call
// that needs the stream), or by itself after EKF_STREAM_IDLE_TICKS without a command.
//   host -> device: StreamCmd, seventeen self-validating granules (record and flags), each tagged with the command's sequence number
//   device -> host: StreamCtl::state = (launch number << 2) | phase, and the mirror
// Leaving by itself races with a command being posted; both sides do "write mine, fence, read yours" (the host: command, mfence,
// state; workgroup 0: state = EXITING, system fence, command slot -- a PCIe read does not pass the posted write in front of it), so at
// least one sees the other: workgroup 0 cancels its exit when it finds a command, the host waits for the outcome when it finds
// EXITING, and relaunches when the kernel has left without consuming the command.
#define EKF_STREAM_RING 16
#define EKF_STREAM_IDLE_TICKS 10000 /* of the 100 MHz clock: 100 us */
enum { EKF_STREAM_RUNNING = 1, EKF_STREAM_EXITING = 2, EKF_STREAM_EXITED = 3 };
enum { EKF_STREAM_END_AFTER = 1, EKF_STREAM_EXIT = 2 };  // command flags: leave after this operation (host); leave now (workgroup 0's forward only)
struct alignas(128) StreamCmd {
    // Seventeen self-validating 8-byte granules {32 payload bits, 32-bit tag = the low half of the command's sequence number} -- the form the
    // cross-workgroup exchange uses (MI355X_MICROARCH.md, granules): g[0] = the flags, g[1 + 2i], g[2 + 2i] = low / high half of rec[i].  The
    // host writes g[0] last and the launch polls it (with the rest of the command's first cache line) -- but nothing DEPENDS on that order:
    // every granule is re-read until it carries the tag, so no assumption is made about the order in which reads of two cache lines of host
    // memory are served.
    unsigned long long g[18];
};
struct alignas(128) StreamCtl {
    unsigned long long state;  // written by workgroup 0: (launch << 2) | EKF_STREAM_*
    unsigned long long consumed;  // ... with EXITED: the last command the launch consumed
    unsigned long long pad0[14];
    unsigned long long stop;   // written by the host: launch number that shall leave now
    unsigned long long pad1[15];
    StreamCmd cmd[EKF_STREAM_RING];
};

struct EkfDev {
    int B, Ncap;
    int xs;    // stride of x and of each R row (doubles), multiple of 64, >= 3 + 2*Ncap
    int dn;    // stride of each D component, = 32*T
    int T;     // 64x64 tiles per side of P_LL
    int maxp;  // slots (measurements) per set
    int maxpairs;  // (maxp + 1) / 2 slot pairs per set; pair maxpairs is all zeros
    int vs_cap;    // virtual slots per 64-landmark chunk of k_chain's own-row cache in LDS: maxp (in place) or 2 * maxp (overlap)
    int logcap;
    int rows;  // 64*T: rows of one slot in FA / FB
    int lpw;   // landmarks owned by one k_chain workgroup
    int gmax;  // k_chain workgroups per filter
    int hpw;   // k_chain<true>: arg-min heads (and records) a workgroup publishes per exchange = its owner waves, ceil(lpw / 64); else 1
    int nrec;  // gmax * hpw <= 64: records per filter and exchange parity in `part`
    size_t bm_stride;  // doubles per filter in one Bm buffer: T(T+1)/2 * 4096
    size_t f_stride;   // doubles per (filter, set) in FA / FB: (maxpairs + 1) * rows * 4
    double *x, *R, *D;
    double *Bm[2];
    double *FA, *FB;   // [B][2][f_stride]
    int *n_lm, *n_lm_sweep, *status;
    int *n_lm_flush;   // [B][2]: landmark count when set s was last written (sizes its dense pass)
    int *slot_active;  // [B][2][maxp]
    SlotMeta *slot_meta;  // [B][2][maxp], written with the slot
    int *pass_flag;    // [1]: number of dense passes completed (overlap mode; stored by k_mark behind each pass)
    unsigned long long *seg_count;  // [EKF_PLAN_MAX]: counter i = workgroups that have finished segment i of the handle's multi-segment chain launches
                                    // (all launches so far).  One counter PER SEGMENT: workgroups of different filters -- and of one filter, in a
                                    // segment without an exchange -- do not wait for each other between segments, so a sum over segments could reach
                                    // "every workgroup, segment s" while one workgroup is still inside s.  The dense pass of segment i sits behind
                                    // hipStreamWaitValue64(seg_count[i] >= ChainSeg::gate)
    int *bar;          // [B][2]: [0] = cross-workgroup exchanges done so far (tags of the records continue from it)
    long long *dbg;    // [32] diagnostics: tick counters of the control lane [0..7] and of the first worker [16..23] (EKF_CHAIN_STAMPS), first bad index [8..11] (EKF_CHAIN_CHECK)
    double *part;      // [B][2][nrec][EKF_REC_DOUBLES]: arg-min records (per workgroup; k_chain<true>: per owner wave), double-buffered by exchange parity
    StreamCtl *sctl;   // streaming launches (one-filter handles): the host-mapped block whose state word and consumed count the launch writes, device view
    StreamCtl *sring;  // ... and the block whose command ring and stop word the host writes and the launch polls: DEVICE memory (fine-grained) the host
                       // writes through the PCIe BAR where the device has a large BAR -- a poll is a local read instead of a read of host memory across
                       // PCIe (scripts/micro/bar_lab.hip: 0.5 us per trip, and reads of several lines overlap) -- else the same host-mapped block as sctl
    unsigned long long *sfw;  // [32 granules + 1]: workgroup 0's forward of the current command to the filter's other workgroups (10 values as tagged
                              // 16-byte granule pairs), [32] = how many workgroups have read a forward so far (all launches)
    ekf_decision *log;
    long long *log_count;
    ekf_stats *stats;
    EkfMirror *mirror;  // [B], host-mapped
    double gamma_max, gamma_min, cond_limit;
    long long spin_limit;  // polls of the in-kernel pass wait before a launch gives up (EKF_ERR_TIMEOUT)
    double cond_k2;  // ((L^2 - 1) / (2 (L^2 + 1)))^2 for L = cond_limit: the sweep's condition test without sqrt / division
};

// Offset (doubles) of P_LL element (i', j') inside one filter's Bm.  Requires tile(i') <= tile(j');
// callers outside a diagonal tile pass i' <= j'.  Tile (I, J), J >= I, is the
// (I*T - I(I-1)/2 + J - I)-th 4096-double tile.  Inside a tile, 16 chains (row16-block rc, col16-
// block cc) of 256 doubles; a chain is the C/D operand of v_mfma_f64_16x16x4_f64 stored as two
// wave-contiguous 1 KiB pieces: piece h holds registers 2h, 2h+1 of every lane, lane = 16*(row&3)
// + col, register = row>>2.  bm_tile_base: the offset of stored tile (I, J), I <= J < T, alone.
__host__ __device__ inline size_t bm_tile_base(int T, int I, int J) {
    return ((size_t)I * T - ((size_t)I * (I - 1)) / 2 + (size_t)(J - I)) * 4096;
}
__host__ __device__ inline size_t bm_offset(int T, int ip, int jp) {
    int I = ip >> 6, J = jp >> 6;
    size_t t = (size_t)I * T - ((size_t)I * (I - 1)) / 2 + (size_t)(J - I);  // (= bm_tile_base / 4096, kept in its own words: the hot kernels' code follows them)
    int il = ip & 63, jl = jp & 63;
    int chain = (il >> 4) * 4 + (jl >> 4);
    int rho = il & 15, c = jl & 15;
    int r = rho >> 2, g = rho & 3;
    return t * 4096 + (size_t)chain * 256 + (size_t)(r >> 1) * 128 + (size_t)(g * 16 + c) * 2 + (r & 1);
}

// Tiles per side of the P_LL of n landmarks: the tile of the last landmark row, 2n - 1, plus one.
__host__ __device__ inline int lm_tiles(int n) { return (2 * n + 63) >> 6; }

// The inverse of bm_offset inside one tile: tile-local offset o (0..4095) -> tile-local row il, column jl.
__host__ __device__ inline void bm_tile_coords(int o, int *il, int *jl) {
    const int chain = o >> 8, h = (o >> 7) & 1, lane = (o >> 1) & 63, e = o & 1;
    *il = (chain >> 2) * 16 + (lane >> 4) + 4 * (2 * h + e);
    *jl = (chain & 3) * 16 + (lane & 15);
}

// Landmark removal (ekf_remove_landmarks) gathers by destination.  map[l'] = old number of kept landmark l' (increasing), n_new kept
// landmarks: landmark-space row i' of the reduced map is old row remove_row(...), or -1 beyond the reduced map.
__host__ __device__ inline int remove_row(const int *map, int n_new, int ip) {
    return ip < 2 * n_new ? 2 * map[ip >> 1] + (ip & 1) : -1;
}

// Where element (i', j') of the reduced P_LL comes from, given its old rows si = remove_row(i'), sj = remove_row(j'): exactly what
// k_import of the dense export with the rows and columns deleted would store there.  A landmark's own 2x2 block comes from D
// (offset comp * dn + landmark), every other element from the upper-triangle home (min, max) in Bm (map is increasing, so an element of an
// upper-triangle tile reads an upper-triangle tile at or after it in both tile coordinates); beyond the reduced map: zero.
enum { RM_ZERO = 0, RM_BM = 1, RM_D = 2 };
struct RmSource {
    int where;
    size_t off;
};
__host__ __device__ inline RmSource remove_source(int T, int dn, int si, int sj) {
    RmSource s;
    if (si < 0 || sj < 0) {
        s.where = RM_ZERO, s.off = 0;
    } else if ((si >> 1) == (sj >> 1)) {
        s.where = RM_D, s.off = (size_t)((si & 1) + (sj & 1)) * dn + (si >> 1);
    } else {
        s.where = RM_BM, s.off = si < sj ? bm_offset(T, si, sj) : bm_offset(T, sj, si);
    }
    return s;
}

// Frame changes (ekf_transform_frame / ekf_anchor_at_robot) rewrite every off-diagonal 2x2 landmark block of P_LL in place.  A
// tile is 512 WORK ITEMS of eight doubles: item q reads the two 32-byte pieces at tile-local offsets off and off + 32 (bm_offset:
// +32 doubles = the next row, +2 = the next column, +1 = four rows down), which are exactly two complete 2x2 blocks -- rows
// (row[k], row[k] + 1) x columns (col, col + 1) for k = 0, 1 -- so no value crosses a lane.  Value v (0..3) of piece s (0..1) is
// element (row[v & 1] + s, col + (v >> 1)).  64 consecutive items (one wave) cover two whole chains; 16 consecutive items one 1 KiB
// piece of a chain, as two interleaved 256-byte runs per load.
struct ReframeItem {
    int off;     // tile-local offset (doubles) of the first piece; the second is at off + 32
    int row[2];  // tile-local first (even) row of block 0 and of block 1 (= row[0] + 4)
    int col;     // tile-local first (even) column of both blocks
    int chain;   // the item's chain: (row16-block << 2) | col16-block
};
__host__ __device__ inline ReframeItem reframe_item(int q) {
    ReframeItem it;
    const int chain = q >> 5, h = (q >> 4) & 1, gp = (q >> 3) & 1, c2 = q & 7;
    it.chain = chain;
    it.off = chain * 256 + h * 128 + gp * 64 + c2 * 4;
    it.row[0] = (chain >> 2) * 16 + 8 * h + 2 * gp;
    it.row[1] = it.row[0] + 4;
    it.col = (chain & 3) * 16 + 2 * c2;
    return it;
}
// Offset inside a chain (0..255) of element (rho, c) of its 16x16 block: bm_offset without the tile and chain terms.
__host__ __device__ inline int bm_chain_offset(int rho, int c) {
    const int r = rho >> 2, g = rho & 3;
    return (r >> 1) * 128 + (g * 16 + c) * 2 + (r & 1);
}

// (I, J) of stored tile t of a triangle with side nT, in storage order (t = I*nT - I(I-1)/2 + J - I): the grid of the kernels that
// take one workgroup per tile (removal, frame changes)
__host__ __device__ inline void tri_tile_ij(int t, int nT, int *I, int *J) {
    int i = 0;
    while (t >= nT - i) t -= nT - i, i++;
    *I = i, *J = i + t;
}

// Map joining (ekf_join_map) appends the Ns landmarks of a source filter behind the Ng landmarks of the destination: only the tile
// COLUMNS from J0 = Ng / 32 on hold a new column, and one workgroup rewrites each of their tiles (I <= J), gathered by destination.
// Tile t of that list (column after column) is (I, J); false behind the last column J1 - 1, J1 = tiles per side of the joined map.
__host__ __device__ inline bool join_tile_ij(int t, int J0, int J1, int *I, int *J) {
    int j = J0;
    while (j < J1 && t >= j + 1) t -= j + 1, j++;
    *I = t, *J = j;
    return j < J1;
}
__host__ __device__ inline int join_tile_count(int Ng, int Ns) {
    const int J0 = Ng >> 5, J1 = lm_tiles(Ng + Ns);
    return Ns > 0 ? J1 * (J1 + 1) / 2 - J0 * (J0 + 1) / 2 : 0;
}

// Landmark initialisation (ekf_add_landmarks) walks the same tile columns with a measurement table in place of a source filter: a
// filter's record is {count, 0} and then zcap entries of six doubles {z_x, z_y, R00, R10, R01, R11}; its stride in doubles, a
// multiple of four (what lies behind the table stays 32-byte aligned).
__host__ __device__ inline size_t add_tab_stride(int zcap) { return (2 + 6 * (size_t)zcap + 3) & ~(size_t)3; }

// Where element (i', j') of the joined P_LL (landmark space, either order) comes from.  The SOURCE filter has a layout of its own
// (Ts tiles per side, D stride dns: its capacity's, not the destination's).
//   JM_OLD    both landmarks are the destination's: the element stays, bit for bit
//   JM_ROBOT  one old, one new landmark: P_mR G_k^T, from the destination's robot rows alone (no source element)
//   JM_BM     two different new landmarks: G_k P_RR G_l^T + (C P_s,kl C^T), the source block's upper-triangle home in the source's Bm;
//             si, sj = the element's own rows in the source's landmark space (the rotation mixes it with the three others of its
//             2x2 block, which lie at off(2k + e, 2l + f) = off(2k, 2l) + 32 e + 2 f: a landmark's two rows never leave a chain)
//   JM_D      a new landmark's own block: the source's D (offset comp * dns + landmark)
//   JM_ZERO   beyond the joined map
enum { JM_ZERO = 0, JM_OLD = 1, JM_ROBOT = 2, JM_BM = 3, JM_D = 4 };
// ... of the block (landmark li, landmark lj) alone: all that ekf_add_landmarks' tile kernel needs (its new landmarks have no source
// layout: Ns = the number of additions).  join_source below keeps its own words for the same cases -- written through this function,
// k_join_tiles came out with 70 instead of 63 VGPRs and one wave per SIMD less, and the join's code is to stay as it was measured --;
// tests/cpp/add_plan_check.cpp holds the two to each other.
__host__ __device__ inline int join_where(int Ng, int Ns, int li, int lj) {
    if (li >= Ng + Ns || lj >= Ng + Ns) return JM_ZERO;
    if (li < Ng && lj < Ng) return JM_OLD;
    if (li < Ng || lj < Ng) return JM_ROBOT;
    return li == lj ? JM_D : JM_BM;
}
struct JoinSource {
    int where;
    int si, sj;  // JM_BM / JM_D: rows of the source's landmark space, in the order asked for
    size_t off;  // JM_BM: into the source filter's Bm, element (min, max); JM_D: into its D
};
__host__ __device__ inline JoinSource join_source(int Ng, int Ns, int Ts, int dns, int ip, int jp) {
    JoinSource s;
    s.where = JM_ZERO, s.si = s.sj = -1, s.off = 0;
    const int li = ip >> 1, lj = jp >> 1;
    if (li >= Ng + Ns || lj >= Ng + Ns) return s;
    if (li < Ng && lj < Ng) {
        s.where = JM_OLD;
    } else if (li < Ng || lj < Ng) {
        s.where = JM_ROBOT;
    } else {
        s.si = ip - 2 * Ng, s.sj = jp - 2 * Ng;
        if (li == lj) s.where = JM_D, s.off = (size_t)((s.si & 1) + (s.sj & 1)) * dns + (s.si >> 1);
        else s.where = JM_BM, s.off = s.si < s.sj ? bm_offset(Ts, s.si, s.sj) : bm_offset(Ts, s.sj, s.si);
    }
    return s;
}

// The tile-blocked Cholesky of P_LL (ekf_joint_consistency, ekf_factor.hip).  Step k updates the stored tiles (I, J) with
// k < I <= J < nT: tile t of that list, in storage order of the triangle that is left, and their number.
__host__ __device__ inline int chol_trail_count(int nT, int k) {
    const int m = nT - 1 - k;
    return m > 0 ? m * (m + 1) / 2 : 0;
}
__host__ __device__ inline void chol_trail_ij(int t, int nT, int k, int *I, int *J) {
    tri_tile_ij(t, nT - 1 - k, I, J);
    *I += k + 1, *J += k + 1;
}
// A stored chain is an operand of v_mfma_f64_16x16x4_f64 as it lies: in k-step s (0..15) of the product U_ki^T U_kj, lane l holds
// element (row 4 s + (l >> 4), column 16 blk + (l & 15)) of a panel tile -- as A for output row block blk, as B for output column
// block blk.  Its tile-local offset; s even: the lane's 16-byte piece at that offset carries k-steps s and s + 1.
__host__ __device__ inline int chol_operand_offset(int s, int blk, int lane) {
    return ((s >> 2) * 4 + blk) * 256 + ((s >> 1) & 1) * 128 + lane * 2 + (s & 1);
}

// Duplicate search (ekf_find_duplicates, ekf_pairs.hip): the pairs of landmarks i < j < n a call considers, walked by stored tile
// (32 x 32 landmarks), work item (reframe_item: two complete cross blocks P_ij) and block.  split = 0: every pair, i.e. the stored
// triangle of side lm_tiles(n).  0 < split <= n: only i < split <= j, which live in the rectangle of tiles I <= (split - 1) / 32,
// J >= split / 32 (I <= J there); the two straddling tile rows / columns are filtered per pair.
__host__ __device__ inline int dup_tile_count(int n, int split) {
    const int nT = lm_tiles(n);
    if (n < 2 || split >= n) return 0;
    if (split <= 0) return nT * (nT + 1) / 2;
    return (((split - 1) >> 5) + 1) * (nT - (split >> 5));
}
// tile t of that list; false behind its end
__host__ __device__ inline bool dup_tile_ij(int t, int n, int split, int *I, int *J) {
    if (t < 0 || t >= dup_tile_count(n, split)) return false;
    const int nT = lm_tiles(n);
    if (split <= 0) {
        tri_tile_ij(t, nT, I, J);
    } else {
        const int J0 = split >> 5, w = nT - J0;
        *I = t / w, *J = J0 + t % w;
    }
    return true;
}
// block k (0, 1) of work item `it` of tile (I, J): the pair it holds, or false (beyond the map, not above the diagonal -- a
// landmark's own block and the below-diagonal twins of a diagonal tile, which are nobody's home -- or on one side of the split)
__host__ __device__ inline bool dup_pair(int n, int split, int I, int J, const ReframeItem &it, int k, int *i, int *j) {
    const int li = 32 * I + (it.row[k] >> 1), lj = 32 * J + (it.col >> 1);
    *i = li, *j = lj;
    return li < lj && lj < n && (split <= 0 || (li < split && lj >= split));
}
// The Euclidean bound: squared distance in ONE written-out form (a fused multiply-add, on the host and on the device), used for
// the pairs and for the gaps between two groups' bounding boxes alike.  Rounding is monotone, so a box gap that is no larger than
// every |L_i - L_j| component of the tile gives a value no larger than any pair's: a culled tile holds no pair within the bound.
__host__ __device__ inline double dup_dist2(double dx, double dy) { return __builtin_fma(dx, dx, dy * dy); }
__host__ __device__ inline double dup_box_gap(double lo_a, double hi_a, double lo_b, double hi_b) {
    const double g0 = lo_a - hi_b, g1 = lo_b - hi_a;
    const double g = g0 > g1 ? g0 : g1;
    return g > 0.0 ? g : 0.0;
}
// The gate of one pair (include/ekfslam_c.h): S = P_ii + P_jj - P_ij - P_ij^T as (a, b; b, c), d = L_i - L_j.  Returns 0 with
// *d2 = d^T S^-1 d, or 1 when the pair is degenerate (S not positive definite, NaN included).  No contraction: the host reference
// (tests/dup_ref.py) evaluates the same operations in the same order.
__host__ __device__ inline int dup_gate(double dx, double dy, const double di[3], const double dj[3], const double pij[4], double *d2) {
#pragma clang fp contract(off)
    const double a = (di[0] + dj[0]) - 2.0 * pij[0];
    const double b = ((di[1] + dj[1]) - pij[1]) - pij[2];
    const double c = (di[2] + dj[2]) - 2.0 * pij[3];
    const double det = a * c - b * b;
    if (!(a > 0.0 && det > 0.0)) return 1;
    *d2 = ((c * dx * dx - 2.0 * b * dx * dy) + a * dy * dy) / det;
    return 0;
}

// Offset (doubles) of row i' of slot PAIR p inside one (filter, set) of FA / FB: 4 doubles, slot 2p in
// [0..1], slot 2p+1 in [2..3].
__host__ __device__ inline size_t pair_offset(int rows, int ip, int p) {
    return ((size_t)p * rows + ip) * 4;
}

// Landmark fusion (ekf_fuse_landmarks, ekf_fuse.hip) gathers columns of P: where the 2x2 block (landmark l, landmark c) of P_LL
// lives.  FW_D: l == c, the own block in D (component e + f at (e + f) * dn + l).  FW_BM: l < c, the stored block; `off` is its
// element (0, 0) in the filter's Bm, element (e, f) at off + 32 e + 2 f.  FW_BM_T: l > c, the block is the transpose of the stored
// (c, l): element (e, f) at off + 32 f + 2 e.  The two rows of a landmark never leave a chain, and a 32-byte piece holds rows rho and
// rho + 4 of two columns: the block's aligned pieces start at off - (off & 1) and 32 doubles on, the block is half (off & 1) of them
// (reframe_item: row[0] and row[1]).
enum { FW_D = 0, FW_BM = 1, FW_BM_T = 2 };
struct FuseSource {
    int where;
    size_t off;
};
__host__ __device__ inline FuseSource fuse_source(int T, int l, int c) {
    FuseSource s;
    if (l == c) s.where = FW_D, s.off = (size_t)l;
    else if (l < c) s.where = FW_BM, s.off = bm_offset(T, 2 * l, 2 * c);
    else s.where = FW_BM_T, s.off = bm_offset(T, 2 * c, 2 * l);
    return s;
}
// Column q (0 .. 2m - 1) of a fusion round -- component q & 1 of pair q >> 1 -- is element q & 3 of slot pair q >> 2: the offset
// (doubles) of W / V element (row i', column q) inside set 0 of FA / FB.
__host__ __device__ inline size_t fuse_slot_offset(int rows, int ip, int q) { return pair_offset(rows, ip, q >> 2) + (size_t)(q & 3); }

// Submap extraction (ekf_extract_map, ekf_get_submap; ekf_extract.hip) gathers by destination, from a source filter with a layout
// of its own (Ts tiles per side, D stride dns).  ids[k] = source landmark of destination landmark k, pairwise distinct, in ANY
// order; `count` landmarks are extracted.  extract_landmark: the source landmark of destination landmark k, -1 beyond the new map.
// extract_block: where the 2x2 block (destination landmarks k, m) = P(a, c) of the source lives, a = ids[k], c = ids[m] -- its own
// block in D, the stored block, or the stored block (c, a) transposed (fuse_source: the order of the ids decides, not the order
// of k and m, so a place below the diagonal of a diagonal tile gets what k_import stores there) --, EX_ZERO beyond the new map.
// extract_element: the same for one element (i', j') of the destination's landmark space, for the dense read-out: the removal's
// rule with ids in place of its increasing map (remove_source takes (min, max) of the source rows itself).
enum { EX_ZERO = -1 };  // beside FW_D, FW_BM, FW_BM_T
__host__ __device__ inline int extract_landmark(const int *ids, int count, int k) { return k < count ? ids[k] : -1; }
__host__ __device__ inline FuseSource extract_block(int Ts, int a, int c) {
    if (a < 0 || c < 0) {
        FuseSource s;
        s.where = EX_ZERO, s.off = 0;
        return s;
    }
    return fuse_source(Ts, a, c);
}
__host__ __device__ inline RmSource extract_element(int Ts, int dns, const int *ids, int count, int ip, int jp) {
    return remove_source(Ts, dns, remove_row(ids, count, ip), remove_row(ids, count, jp));
}
