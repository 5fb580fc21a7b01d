// ekf_map_api.hip -- host side of the map operations of include/ekfslam_c.h: removal, frame change and anchoring, joining, extraction
// and ekf_get_submap, joint consistency, duplicate search, fusion, matched updates and their score, the individual compatibility table,
// the joint compatibility search, landmark initialisation and the scan step built from those, relocalisation (the pose search, the
// pose reset and the two with a matched update), ekf_get_landmark_covs.  Included
// by ekf_api.hip (one translation unit: ekf_batch, HIP_TRY / EKF_TRY, quiesce, finish_rewrite, DevTmp, HostCopies and MapKept are
// that file's).  Every entry point runs once per call on a handle it brings to rest and reads: check, quiesce, plan, upload, launch,
// finish.  The checks of the caller's lists and the tables the kernels read are pure code in ekf_map_plan.h; the order of those
// checks relative to quiescing is the table above quiesce().  Every asynchronous copy that touches a local buffer or a caller's goes
// through a HostCopies guard declared behind those buffers.
// Adding a kept block: (1) its struct and carve function in ekf_map_scratch.h (and a case in tests/cpp/map_scratch_check.cpp); (2) a
// BLK_ value, a member and a row of the table of MapKept (ekf_api.hip), and a line in map_scratch_rebuild if ekf_reserve is to build
// it again; (3) a block_build call where the operation finds the block absent or too small.

// The filters of a call, [b0, b0 + nb) of a handle: one filter, or (index < 0) the whole batch; and their landmark counts (h_int[]).
struct Filters {
    int b0, nb;
};
static Filters filters_of(const ekf_batch *h, int index) { return index < 0 ? Filters{0, h->dv.B} : Filters{index, 1}; }
static const int *counts_of(const ekf_batch *h, int b0) { return h->h_int.data() + b0; }

// A block of device scratch for the handle to keep (DevBlock), optionally zeroed on the chain stream and waited for; a failure
// leaves *blk as it was.  A block that *blk held goes once the new one exists.
static int block_alloc(ekf_batch *h, DevBlock *blk, size_t bytes, bool zero) {
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    hipError_t e = zero ? hipMemsetAsync(p, 0, bytes, h->s_chain) : hipSuccess;
    if (zero && e == hipSuccess) e = stream_wait(h->s_chain);
    if (e != hipSuccess) {
        hipFree(p);
        return set_error(EKF_ERR_HIP, "%s", hipGetErrorString(e));
    }
    if (blk->p) hipFree(blk->p);
    h->device_bytes += bytes - blk->bytes;
    blk->p = p, blk->bytes = bytes;
    return EKF_OK;
}
// Block `id` of h->map built (again) for scratch struct *sc by its carve function of ekf_map_scratch.h: sized by a carve without a
// base (into a copy: a failure leaves *sc as it was, too), allocated, carved.
template <typename S, typename... Cap>
static int block_build(ekf_batch *h, int id, bool zero, S *sc, void (*carve)(S &, Carver &, const ScratchGeom &, Cap...), Cap... cap) {
    const EkfDev &dv = h->dv;
    const ScratchGeom g = {(size_t)dv.B, dv.Ncap, (size_t)dv.rows, (size_t)dv.xs, (size_t)dv.dn, dv.bm_stride};
    S probe = *sc;
    Carver size{nullptr};
    carve(probe, size, g, cap...);
    EKF_TRY(block_alloc(h, &h->map.blk[id], size.bytes(), zero));
    Carver at{(char *)h->map.blk[id].p};
    carve(*sc, at, g, cap...);
    return EKF_OK;
}

// Each operation's scratch, asked for by every call that needs it: built where it is absent or, where it follows what calls bring
// (n_meas entries of a list, `cap` / `cand` entries found), outgrown.  Which block follows what: the table of MapKept.
static int factor_reserve(ekf_batch *h) {
    if (h->map.blk[BLK_FACTOR].p) return EKF_OK;
    h->fac_stamp[0] = -1;
    return block_build(h, BLK_FACTOR, /*zero*/ true, &h->map.fac, carve_factor);
}
static int dup_reserve(ekf_batch *h, int cap) {
    if (!h->map.blk[BLK_DUP].p) EKF_TRY(block_build(h, BLK_DUP, /*zero*/ true, &h->map.dup, carve_dup));
    return cap > h->map.dup.cap ? block_build(h, BLK_DUP_LIST, /*zero*/ false, &h->map.dup, carve_dup_list, cap) : EKF_OK;
}
static int fuse_reserve(ekf_batch *h) { return h->map.blk[BLK_FUSE].p ? EKF_OK : block_build(h, BLK_FUSE, /*zero*/ true, &h->map.fuse, carve_fuse); }
static int match_reserve(ekf_batch *h, int n_meas) {
    const int zcap = plan_grown_cap(h->map.match.zcap, n_meas, 64);
    if (h->map.blk[BLK_MATCH].p && zcap == h->map.match.zcap) return EKF_OK;
    return block_build(h, BLK_MATCH, /*zero*/ true, &h->map.match, carve_match, zcap);
}
static int iter_reserve(ekf_batch *h, int n_meas) {
    const int zcap = plan_grown_cap(h->map.iter.zcap, n_meas, 64);
    if (h->map.blk[BLK_ITER].p && zcap == h->map.iter.zcap) return EKF_OK;
    return block_build(h, BLK_ITER, /*zero*/ true, &h->map.iter, carve_iter, zcap);
}
static int gate_reserve(ekf_batch *h, int n_meas, int cand) {
    GateScratch &gs = h->map.gate;
    const int zcap = plan_grown_cap(gs.zcap, n_meas, 64);
    if (!h->map.blk[BLK_GATE].p || zcap != gs.zcap) EKF_TRY(block_build(h, BLK_GATE, /*zero*/ true, &gs, carve_gate, zcap));
    return cand > gs.ccap ? block_build(h, BLK_GATE_LIST, /*zero*/ false, &gs, carve_gate_list, cand) : EKF_OK;
}
static int assoc_reserve(ekf_batch *h) { return h->map.blk[BLK_ASSOC].p ? EKF_OK : block_build(h, BLK_ASSOC, /*zero*/ true, &h->map.assoc, carve_assoc); }
static int add_reserve(ekf_batch *h, int n_meas) {
    const int zcap = plan_add_zcap(h->map.add.zcap, n_meas);
    if (h->map.blk[BLK_ADD].p && zcap == h->map.add.zcap) return EKF_OK;
    return block_build(h, BLK_ADD, /*zero*/ true, &h->map.add, carve_add, zcap);
}
static int loc_reserve(ekf_batch *h, int cand) {
    LocScratch &ls = h->map.loc;
    if (!h->map.blk[BLK_LOC].p) EKF_TRY(block_build(h, BLK_LOC, /*zero*/ true, &ls, carve_loc));
    return cand > ls.ccap ? block_build(h, BLK_LOC_LIST, /*zero*/ false, &ls, carve_loc_list, cand) : EKF_OK;
}
// The entries of a device list (pairs, candidates) for a call that may hand out up to `want` of them (a call that finds more grows it).
static int list_cap_for(int want) { return plan_grown_cap(0, want < 4096 ? want : 4096, 256); }

// ekf_reserve: `old` is what the smaller buffers had (its pointers are gone); the rule is in the table of MapKept.
static int map_scratch_rebuild(ekf_batch *h, const MapKept &old) {
    if (old.blk[BLK_FACTOR].p) EKF_TRY(factor_reserve(h));
    if (old.blk[BLK_DUP_LIST].p) EKF_TRY(dup_reserve(h, old.dup.cap));
    if (old.blk[BLK_FUSE].p) EKF_TRY(fuse_reserve(h));
    if (old.blk[BLK_MATCH].p) EKF_TRY(match_reserve(h, old.match.zcap));
    if (old.blk[BLK_ITER].p) EKF_TRY(iter_reserve(h, old.iter.zcap));
    if (old.blk[BLK_GATE].p) EKF_TRY(gate_reserve(h, old.gate.zcap, old.gate.ccap));
    if (old.blk[BLK_ASSOC].p) EKF_TRY(assoc_reserve(h));
    if (old.blk[BLK_ADD].p) EKF_TRY(add_reserve(h, old.add.zcap));
    if (old.blk[BLK_LOC].p) EKF_TRY(loc_reserve(h, old.loc.ccap));
    return EKF_OK;
}

// ---- map management -------------------------------------------------------------------------------
// Marginalise landmarks out on the device: gather by destination over the tile layout (k_rm_gather), in overlap mode into the other Bm
// buffer (then flipped, as settle() does behind a pass; the buffer read is cleared), in place through a transient scratch copied back
// (k_rm_finish); x, R, D compacted by k_rm_vec.  Every buffer ends as ekf_set_state of the reduced state would leave it; the buffer
// addresses do not change (captured graphs and streaming launches hold EkfDev by value).
// The removal itself, on a handle that quiesce(QUIET_SETTLED) has brought to rest (h_int[] current): remove_impl, and the end of
// ekf_fuse_landmarks behind its own kernels on the chain stream.  Filter f.b0 + k has the mask keep + k * ld_keep; its new count
// goes to n_out[k] (n_out may be null).
static int remove_settled(ekf_batch *h, Filters f, const unsigned char *keep, int ld_keep, int *n_out) {
    EkfDev &dv = h->dv;
    const int B = dv.B, mstride = dv.Ncap > 0 ? dv.Ncap : 1;
    const RemovalPlan pl = plan_removal(counts_of(h, 0), B, mstride, keep, ld_keep, f.b0, f.nb);
    for (int k = 0; n_out && k < f.nb; k++) n_out[k] = pl.n_new(f.b0 + k);
    if (!pl.any) return EKF_OK;
    const int nTo = pl.nTo, nTn = pl.nTn;
    hipStream_t s = h->s_chain;
    DevTmp<int> rm_d;
    DevTmp<double> scratch;
    const size_t scratch_stride = (size_t)nTn * (nTn + 1) / 2 * 4096;
    HostCopies hc(s);
    if (!h->overlap && scratch_stride) HIP_TRY(scratch.alloc((size_t)B * scratch_stride));
    HIP_TRY(hc.upload(&rm_d, pl.rm.data(), pl.rm.size()));
    if (nTo > 0) {
        const dim3 grid((unsigned)(nTo * (nTo + 1) / 2), (unsigned)B);
        if (h->overlap) {
            hipLaunchKernelGGL(k_rm_gather, grid, dim3(256), 0, s, dv, h->win.buf_in, (const int *)rm_d.p, mstride, nTo, dv.Bm[h->win.buf_in ^ 1], dv.T, dv.bm_stride, 0);
            hipLaunchKernelGGL(k_rm_finish, grid, dim3(256), 0, s, dv, h->win.buf_in, (const int *)rm_d.p, nTo, (const double *)nullptr, 0, (size_t)0);
        } else {
            if (scratch.p)
                hipLaunchKernelGGL(k_rm_gather, grid, dim3(256), 0, s, dv, h->win.buf_in, (const int *)rm_d.p, mstride, nTo, scratch.p, nTn, scratch_stride, 1);
            hipLaunchKernelGGL(k_rm_finish, grid, dim3(256), 0, s, dv, h->win.buf_in, (const int *)rm_d.p, nTo, (const double *)scratch.p, nTn, scratch_stride);
        }
    }
    // D is read by the gather (landmarks' own blocks): compacted behind it
    hipLaunchKernelGGL(k_rm_vec, dim3(7, B), dim3(1024), 0, s, dv, (const int *)rm_d.p, mstride);
    EKF_TRY(finish_rewrite(h, 0, B, /*rearm*/ true, &pl.rm[1], 2, /*flip_buf: the gather's output*/ h->overlap && nTo > 0));
    hc.waited();
    return EKF_OK;
}

static int remove_impl(ekf_batch *h, Filters f, const unsigned char *keep, int ld_keep, int *n_out) {
    // h_int[b] = landmarks of filter b; a sticky EKF_ERR_TIMEOUT or EKF_ERR_CAPACITY ends it here: the state stays as it is; then
    // every deferred slot folded, both streams idle
    EKF_TRY(quiesce(h, QUIET_SETTLED, ST_INVALID_OR_FULL));
    return remove_settled(h, f, keep, ld_keep, n_out);
}

extern "C" int ekf_remove_landmarks(ekf_handle h, int index, const unsigned char *keep, int count) {
    if (!filter_ok(h, index) || !keep || count < 0) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    int n;
    EKF_TRY(remove_impl(h, filters_of(h, index), keep, count, &n));
    return n;
}

extern "C" int ekf_batch_remove_landmarks(ekf_handle h, const unsigned char *keep, int ld_keep, int *n_out) {
    if (!h || !keep || ld_keep < 0) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return remove_impl(h, filters_of(h, -1), keep, ld_keep, n_out);
}

// The per-filter argument of a rewrite launch over nb filters (ekf_rewrite.hip: arg_value), vals = [nb][doubles of A]: a one-filter
// call carries it in the kernel arguments (*one), a batch call in a transient table (copied synchronously: vals may leave scope).
template <typename A>
static int rewrite_arg(const std::vector<double> &vals, int nb, A *one, DevTmp<double> *tab) {
    if (nb == 1) memcpy(one, vals.data(), sizeof(A));
    else HIP_TRY(tab->upload(vals.data(), vals.size(), nullptr, /*async*/ false));
    return EKF_OK;
}

// Frame changes on the device (ekf_rewrite.hip: k_reframe_vec, k_reframe_tiles, k_reframe_finish), the order of steps as in
// remove_impl.  frames == nullptr: anchor at the robot; else one (t_x, t_y, theta) per filter of the launch, one launch sequence
// with the grid over the filters.  Bm is rewritten in place in the settled buffer (either pipeline
// mode: no second buffer, no scratch); the only transient allocation is the BATCH rigid call's frame table (48 bytes per filter; a
// one-filter call carries its frame in the kernel arguments); the anchor's per-row operands use slot set 0 of FA / FB, which are
// cleared afterwards as a removal clears them.
static int reframe_impl(ekf_batch *h, Filters f, const double *frames) {
    // h_int[b] = landmarks of filter b; a sticky EKF_ERR_TIMEOUT or EKF_ERR_CAPACITY ends it here: the state stays as it is; then
    // every deferred slot folded, both streams idle
    EKF_TRY(quiesce(h, QUIET_SETTLED, ST_INVALID_OR_FULL));
    EkfDev &dv = h->dv;
    const int b_off = f.b0, nb = f.nb, nT = lm_tiles(most_landmarks(counts_of(h, b_off), nb));
    hipStream_t s = h->s_chain;
    DevTmp<double> fr_d;
    ReframeFrame one = {{0.0, 0.0, 1.0, 0.0, 0.0, 0.0}};
    if (frames) {
        std::vector<double> fr((size_t)nb * 6, 0.0);
        for (int k = 0; k < nb; k++) {
            const double *fk = frames + 3 * (size_t)k;
            fr[6 * k] = fk[0], fr[6 * k + 1] = fk[1], fr[6 * k + 2] = cos(fk[2]), fr[6 * k + 3] = sin(fk[2]), fr[6 * k + 4] = fk[2];
        }
        EKF_TRY(rewrite_arg(fr, nb, &one, &fr_d));
    }
    const double *frc = fr_d.p;
    const auto k_vec = frames ? k_reframe_vec<false> : k_reframe_vec<true>;  // <ANCHOR>
    const auto k_tiles = frames ? k_reframe_tiles<false> : k_reframe_tiles<true>;
    const auto k_finish = frames ? k_reframe_finish<false> : k_reframe_finish<true>;
    if (nT > 0) {
        const dim3 gv((unsigned)cdiv(32 * nT, 256), (unsigned)nb), gt((unsigned)(nT * (nT + 1) / 2), (unsigned)nb);
        hipLaunchKernelGGL(k_vec, gv, dim3(256), 0, s, dv, one, frc, b_off);
        hipLaunchKernelGGL(k_tiles, gt, dim3(256), 0, s, dv, h->win.buf_in, one, frc, b_off, nT);
    }
    hipLaunchKernelGGL(k_finish, dim3(nb), dim3(64), 0, s, dv, one, frc, b_off);
    return finish_rewrite(h, b_off, nb, /*rearm*/ true, nullptr, 0, /*flip_buf*/ false);
}

static bool finite3(const double *f) { return __builtin_isfinite(f[0]) && __builtin_isfinite(f[1]) && __builtin_isfinite(f[2]); }

extern "C" int ekf_transform_frame(ekf_handle h, int index, const double frame[3]) {
    if (!filter_ok(h, index) || !frame || !finite3(frame)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return reframe_impl(h, filters_of(h, index), frame);
}

extern "C" int ekf_batch_transform_frame(ekf_handle h, const double *frames) {
    if (!h || !frames) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    for (int b = 0; b < h->dv.B; b++)
        if (!finite3(frames + 3 * (size_t)b)) return set_error(EKF_ERR_BAD_ARG, "a frame is not finite");
    return reframe_impl(h, filters_of(h, -1), frames);
}

extern "C" int ekf_anchor_at_robot(ekf_handle h, int index) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return reframe_impl(h, filters_of(h, index), nullptr);
}

extern "C" int ekf_batch_anchor_at_robot(ekf_handle h) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    return reframe_impl(h, filters_of(h, -1), nullptr);
}

// What the join and extraction kernels read of a source handle at rest.
static JoinSrc join_src_of(const ekf_batch *s) {
    const EkfDev &sd = s->dv;
    return {sd.x, sd.R, sd.D, sd.Bm[s->win.buf_in], sd.n_lm, sd.xs, sd.dn, sd.T, sd.bm_stride};
}

// Map joining on the device (ekf_rewrite.hip: k_join_tiles, k_join_vec, k_join_finish): filter bs0 + k of `s` into filter
// fd.b0 + k of `d`.  Both handles are brought to rest first (the source is only read afterwards, so its own quiescing is all
// that ever happens to it), which also orders their streams: everything runs on the destination's chain stream while the source's
// streams are idle, and the call waits for it.  Bm is rewritten in place in the destination's settled buffer in either pipeline
// mode; the only transient allocation is the batch form's table of cos / sin (16 bytes per filter).
static int join_impl(ekf_batch *d, Filters fd, ekf_batch *s, int bs0) {
    EKF_TRY(quiesce(s, QUIET_SETTLED, ST_INVALID_OR_FULL));
    if (d != s) EKF_TRY(quiesce(d, QUIET_SETTLED, ST_INVALID_OR_FULL));
    EkfDev &dv = d->dv;
    const int bd0 = fd.b0, nb = fd.nb;
    int nt = 0, nv = 0;
    for (int k = 0; k < nb; k++) {
        const int Ng = d->h_int[bd0 + k], Ns = s->h_int[bs0 + k];
        if (Ng + Ns > dv.Ncap) return set_error(plan_no_room(bd0 + k, Ng, Ns, dv.Ncap, "join"));
        nt = std::max(nt, join_tile_count(Ng, Ns));
        nv = std::max(nv, Ng + Ns);
    }
    DevTmp<double> rot_d;
    Rot2 one = {1.0, 0.0};
    // (the host mirror's heading is the device's x[2] bit for bit once the chain stream is idle: every writer of x[0..2] -- the chain
    // kernels, k_set_meta, the finish kernels -- copies the pose into the mirror; a dense pass does not touch it)
    std::vector<double> rot((size_t)nb * 2);
    for (int k = 0; k < nb; k++) rot[2 * k] = cos(d->mirror_h[bd0 + k].pose[2]), rot[2 * k + 1] = sin(d->mirror_h[bd0 + k].pose[2]);
    EKF_TRY(rewrite_arg(rot, nb, &one, &rot_d));
    const JoinSrc sv = join_src_of(s);
    const double *rotc = rot_d.p;
    hipStream_t st = d->s_chain;
    if (nt > 0) hipLaunchKernelGGL(k_join_tiles, dim3((unsigned)nt, (unsigned)nb), dim3(256), 0, st, dv, d->win.buf_in, sv, one, rotc, bd0, bs0);
    if (nv > 0) hipLaunchKernelGGL(k_join_vec, dim3((unsigned)cdiv(nv, 256), (unsigned)nb), dim3(256), 0, st, dv, d->win.buf_in, sv, one, rotc, bd0, bs0);
    hipLaunchKernelGGL(k_join_finish, dim3(nb), dim3(64), 0, st, dv, sv, one, rotc, bd0, bs0);
    return finish_rewrite(d, bd0, nb, /*rearm*/ true, nullptr, 0, /*flip_buf*/ false);
}

extern "C" int ekf_join_map(ekf_handle dst, int dst_index, ekf_handle src, int src_index) {
    if (!filter_ok(dst, dst_index) || !filter_ok(src, src_index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    if (dst == src && dst_index == src_index) return set_error(EKF_ERR_BAD_ARG, "a filter cannot be joined to itself");
    if (dst->device != src->device) return set_error(EKF_ERR_BAD_ARG, "the two handles live on different devices");
    EKF_TRY(join_impl(dst, filters_of(dst, dst_index), src, src_index));
    return dst->h_int[dst_index];
}

extern "C" int ekf_batch_join_map(ekf_handle dst, ekf_handle src) {
    if (!dst || !src || dst == src) return set_error(EKF_ERR_BAD_ARG, "bad argument (two different handles)");
    if (dst->dv.B != src->dv.B) return set_error(EKF_ERR_BAD_ARG, "the two handles have different batch sizes");
    if (dst->device != src->device) return set_error(EKF_ERR_BAD_ARG, "the two handles live on different devices");
    return join_impl(dst, filters_of(dst, -1), src, 0);
}

// ---- submap extraction ----------------------------------------------------------------------------
// Submap extraction on the device (ekf_extract.hip: k_ext_tiles, k_ext_vec): filter bs0 + k of `s` into filter fd.b0 + k of `d`,
// its new count to n_out[k].  ids == nullptr: every landmark of the source in order; else filter k's list is ids + k * ld_ids with
// count[k] entries, checked on the host before any handle is touched (every id non-negative, no id twice) and against the source's
// landmark count once the source is at rest.
// The source comes to rest first and is only read afterwards (sticky EKF_ERR_TIMEOUT ends the call; a sticky EKF_ERR_CAPACITY does
// not: the state is valid); the destination is then treated as ekf_set_state treats it, except that only the tiles and vector
// entries up to the larger of its previous and its new map are written -- everything behind them is zeros already.  Everything runs
// on the destination's chain stream while the source's streams are idle, and the call waits for it.  The only transient allocation
// is the id table (4 bytes per extracted landmark).
static int extract_impl(ekf_batch *d, Filters fd, ekf_batch *s, int bs0, const int *ids, int ld_ids, const int *count, int *n_out) {
    const int bd0 = fd.b0, nb = fd.nb;
    EKF_TRY(set_error(plan_extract_lists(ids, ld_ids, count, bs0, nb)));
    EKF_TRY(quiesce(s, QUIET_STREAM, ST_INVALID));
    int mstride;
    EKF_TRY(set_error(plan_extract_range(ids, ld_ids, count, counts_of(s, bs0), bs0, nb, &mstride)));
    EKF_TRY(settle(s));
    EkfDev &dv = d->dv;
    std::vector<int> ex;
    EKF_TRY(set_error(plan_extract_table(ids, ld_ids, count, counts_of(s, bs0), bd0, nb, mstride, dv.Ncap, &ex)));
    if (d != s) EKF_TRY(quiesce(d, QUIET_SETTLED, ST_NONE));
    {
        // the destination's previous maps: what has to be overwritten.  A timed-out filter's count is not to be trusted: all of it.
        const int rc = refresh_bounds(d);
        if (rc && rc != EKF_ERR_TIMEOUT) return rc;
    }
    std::vector<int> n_dst((size_t)nb);
    for (int k = 0; k < nb; k++) n_dst[k] = d->mirror_h[bd0 + k].status == EKF_ERR_TIMEOUT ? -1 : d->h_int[bd0 + k];
    const int nT = lm_tiles(plan_extract_old_counts(&ex, n_dst.data(), nb, dv.Ncap));
    hipStream_t st = d->s_chain;
    EKF_TRY(restart_waits(d));
    DevTmp<int> ex_d;
    HostCopies hc(st);
    HIP_TRY(hc.upload(&ex_d, ex.data(), ex.size()));
    const JoinSrc sv = join_src_of(s);
    double *other = d->overlap ? dv.Bm[d->win.buf_in ^ 1] : nullptr;
    if (nT > 0)
        hipLaunchKernelGGL(k_ext_tiles, dim3((unsigned)(nT * (nT + 1) / 2), (unsigned)nb), dim3(256), 0, st, dv, d->win.buf_in, other, sv, (const int *)ex_d.p, mstride, nb, nT, bd0,
                           bs0);
    hipLaunchKernelGGL(k_ext_vec, dim3(7, (unsigned)nb), dim3(1024), 0, st, dv, sv, (const int *)ex_d.p, mstride, nb, bd0, bs0);
    EKF_TRY(finish_rewrite(d, bd0, nb, /*rearm*/ true, &ex[1], 2, /*flip_buf*/ false));
    hc.waited();
    for (int k = 0; n_out && k < nb; k++) n_out[k] = ex[2 * k + 1];
    return EKF_OK;
}

extern "C" int ekf_extract_map(ekf_handle dst, int dst_index, ekf_handle src, int src_index, const int *ids, int count) {
    if (!filter_ok(dst, dst_index) || !filter_ok(src, src_index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    if (ids && count < 0) return set_error(EKF_ERR_BAD_ARG, "negative landmark count");
    if (dst == src && dst_index == src_index) return set_error(EKF_ERR_BAD_ARG, "a filter cannot be extracted into itself");
    if (dst->device != src->device) return set_error(EKF_ERR_BAD_ARG, "the two handles live on different devices");
    int n;
    EKF_TRY(extract_impl(dst, filters_of(dst, dst_index), src, src_index, ids, count, &count, &n));
    return n;
}

extern "C" int ekf_batch_extract_map(ekf_handle dst, ekf_handle src, const int *ids, int ld_ids, const int *count, int *n_out) {
    if (!dst || !src || dst == src) return set_error(EKF_ERR_BAD_ARG, "bad argument (two different handles)");
    if (dst->dv.B != src->dv.B) return set_error(EKF_ERR_BAD_ARG, "the two handles have different batch sizes");
    if (dst->device != src->device) return set_error(EKF_ERR_BAD_ARG, "the two handles live on different devices");
    if (ids && (!count || ld_ids < 0)) return set_error(EKF_ERR_BAD_ARG, "a list of ids needs its counts");
    return extract_impl(dst, filters_of(dst, -1), src, 0, ids, ld_ids, count, n_out);
}

// The same marginal to the host: ekf_get_state's rule (the streaming launch leaves; the size alone folds nothing), then the device
// gathers straight into a transient dense staging matrix of (3 + 2 count)^2 and one copy follows.  The filter is only read.
extern "C" int ekf_get_submap(ekf_handle h, int index, const int *ids, int count, double *x_out, double *P_out, int ld) {
    if (!filter_ok(h, index) || count < 0 || (count > 0 && !ids)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    EKF_TRY(set_error(plan_ids_distinct(ids, count, index)));
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_INVALID));
    EKF_TRY(set_error(plan_ids_in_range(ids, count, h->h_int[index], index)));
    const int n = 3 + 2 * count;
    if (!x_out && !P_out) return n;  // (the size alone: nothing is folded)
    if (!x_out || !P_out || ld < n) return set_error(EKF_ERR_BAD_ARG, "bad output buffers");
    EKF_TRY(settle(h));
    hipStream_t s = h->s_chain;
    DevTmp<double> stage;  // transient staging: dense n x n + x
    DevTmp<int> ids_d;
    HostCopies hc(s);
    HIP_TRY(stage.alloc((size_t)n * n + n));
    HIP_TRY(hc.upload(&ids_d, ids, (size_t)count));
    hipLaunchKernelGGL(k_ext_dense, dim3((unsigned)cdiv(n, 256), (unsigned)n), dim3(256), 0, s, join_src_of(h), index, (const int *)ids_d.p, count, stage.p + (size_t)n * n,
                       stage.p, n, n);
    EKF_TRY(read_back_dense(h, stage.p, n, x_out, P_out, ld));
    hc.waited();
    EKF_TRY(check_launch());
    return n;
}

// ---- map assessment -------------------------------------------------------------------------------
// The filters f: the rule of ekf_get_state (the streaming launch leaves, every deferred slot is folded, both streams idle),
// then the settled state is only read: stage, 3 launches per tile step with the grid over the filters, finish, one copy back.
static int joint_impl(ekf_batch *h, Filters f, const double *x_true, int ld_true, ekf_joint *out) {
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_INVALID));
    const int b0 = f.b0, nb = f.nb, n_max = most_landmarks(counts_of(h, b0), nb);
    if (x_true && ld_true < 3 + 2 * n_max) return set_error(EKF_ERR_BAD_ARG, "x_true rows are shorter than the largest state of the call");
    EKF_TRY(settle(h));
    EKF_TRY(factor_reserve(h));
    const EkfDev &dv = h->dv;
    const FactorScratch fs = h->map.fac;
    hipStream_t s = h->s_chain;
    const int have_truth = x_true ? 1 : 0;
    HostCopies hc(s);
    if (x_true)
        HIP_TRY(hc.copy2d(fs.xt + (size_t)b0 * dv.xs, (size_t)dv.xs * sizeof(double), x_true, (size_t)ld_true * sizeof(double), (size_t)(3 + 2 * n_max) * sizeof(double), nb,
                          hipMemcpyHostToDevice));
    const int nT = lm_tiles(n_max);
    if (nT > 0) hipLaunchKernelGGL(k_chol_stage, dim3((unsigned)(nT * (nT + 1) / 2), (unsigned)nb), dim3(256), 0, s, dv, fs, h->win.buf_in, b0, nT, have_truth);
    for (int k = 0; k < nT; k++) {
        hipLaunchKernelGGL(k_chol_diag, dim3((unsigned)nb), dim3(320), 0, s, dv, fs, k, b0);
        if (k + 1 < nT) {
            hipLaunchKernelGGL(k_chol_panel, dim3((unsigned)(nT - 1 - k), (unsigned)nb), dim3(64), 0, s, dv, fs, k, b0);
            hipLaunchKernelGGL(k_chol_trail, dim3((unsigned)chol_trail_count(nT, k), (unsigned)nb), dim3(256), 0, s, dv, fs, k, b0, nT);
        }
    }
    hipLaunchKernelGGL(k_chol_finish, dim3((unsigned)nb), dim3(64), 0, s, dv, fs, b0, have_truth);
    HIP_TRY(hc.copy(out, fs.out + b0, sizeof(ekf_joint) * (size_t)nb, hipMemcpyDeviceToHost));
    HIP_TRY(hc.wait());
    EKF_TRY(check_launch());
    h->fac_stamp[0] = h->chain_seq, h->fac_stamp[1] = h->stream_ops, h->fac_stamp[2] = h->state_edits;
    h->fac_b0 = b0;
    h->fac_n.assign(h->h_int.begin() + b0, h->h_int.begin() + b0 + nb);
    return EKF_OK;
}

extern "C" int ekf_joint_consistency(ekf_handle h, int index, const double *x_true, ekf_joint *out) {
    if (!filter_ok(h, index) || !out) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return joint_impl(h, filters_of(h, index), x_true, x_true ? 3 + 2 * h->dv.Ncap : 0, out);
}

extern "C" int ekf_batch_joint_consistency(ekf_handle h, const double *x_true, int ld_true, ekf_joint *out) {
    if (!h || !out || (x_true && ld_true < 3)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return joint_impl(h, filters_of(h, -1), x_true, ld_true, out);
}

extern "C" int ekf_debug_joint_factor(ekf_handle h, int index, double *U_out, int ld) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    const bool current = h->map.blk[BLK_FACTOR].p && h->fac_stamp[0] == h->chain_seq && h->fac_stamp[1] == h->stream_ops && h->fac_stamp[2] == h->state_edits;
    if (!current || index < h->fac_b0 || index >= h->fac_b0 + (int)h->fac_n.size())
        return set_error(EKF_ERR_STATE, "no factor of this filter's current state: call ekf_joint_consistency first");
    const int m = 2 * h->fac_n[index - h->fac_b0];
    if (m == 0) return 0;
    if (!U_out || ld < m) return set_error(EKF_ERR_BAD_ARG, "bad output buffer");
    HIP_TRY(hipSetDevice(h->device));
    DevTmp<double> stage;
    HIP_TRY(stage.alloc((size_t)m * m));
    hipLaunchKernelGGL(k_chol_export, dim3(cdiv(m, 256), m), dim3(256), 0, h->s_chain, h->dv, h->map.fac, index, m, stage.p, m);
    EKF_TRY(read_back_dense(h, stage.p, m, nullptr, U_out, ld));
    EKF_TRY(check_launch());
    return m;
}

// ---- duplicate search -----------------------------------------------------------------------------
// The filters f: the rule of ekf_get_state (the streaming launch leaves, every deferred slot is folded, both streams idle),
// then the settled state is only read: boxes (with a Euclidean bound), tiles, the counters back, the lists back.  A call that
// finds more pairs than the device list holds and has to hand some out runs the two kernels once more with a list that fits (the
// state has not moved: the same pairs).  The appended order is the hardware's; each filter's list is sorted by (i, j) here.
static int dup_impl(ekf_batch *h, Filters f, double gate, double max_dist, int split_one, const int *split, ekf_dup_pair *pairs_out, int max_pairs, int *n_found_out,
                    int *n_degenerate_out) {
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_INVALID));
    const int b0 = f.b0, nb = f.nb, n_max = most_landmarks(counts_of(h, b0), nb);
    int nt;
    EKF_TRY(set_error(plan_dup_tiles(counts_of(h, b0), b0, nb, split_one, split, &nt)));
    EKF_TRY(settle(h));
    EKF_TRY(dup_reserve(h, list_cap_for(max_pairs)));
    const EkfDev &dv = h->dv;
    hipStream_t s = h->s_chain;
    DupArgs da;
    da.gate = gate, da.md2 = max_dist > 0.0 ? max_dist * max_dist : -1.0, da.split_one = split_one, da.use_tab = split ? 1 : 0;
    std::vector<int> cnt((size_t)2 * nb, 0);
    std::vector<ekf_dup_pair> got;
    HostCopies hc(s);
    if (split && nt > 0) HIP_TRY(hc.copy(h->map.dup.split + b0, split, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice));  // (no tile: no kernel, and nothing waits)
    for (int round = 0; nt > 0; round++) {
        const DupScratch ds = h->map.dup;
        HIP_TRY(hipMemsetAsync(ds.cnt + 2 * (size_t)b0, 0, sizeof(int) * 2 * (size_t)nb, s));
        if (da.md2 >= 0.0) hipLaunchKernelGGL(k_dup_boxes, dim3((unsigned)cdiv(lm_tiles(n_max), 64), (unsigned)nb), dim3(64), 0, s, dv, ds, b0);
        hipLaunchKernelGGL(k_dup_tiles, dim3((unsigned)nt, (unsigned)nb), dim3(256), 0, s, dv, ds, da, h->win.buf_in, b0);
        HIP_TRY(hc.copy(cnt.data(), ds.cnt + 2 * (size_t)b0, sizeof(int) * 2 * (size_t)nb, hipMemcpyDeviceToHost));
        HIP_TRY(hc.wait());
        EKF_TRY(check_launch());
        int most = 0;
        for (int k = 0; k < nb; k++) most = cnt[2 * k] > most ? cnt[2 * k] : most;
        if (most <= ds.cap || max_pairs == 0) break;
        if (round > 0) return set_error(EKF_ERR_STATE, "the pair count changed between two passes over an unchanged state");
        EKF_TRY(dup_reserve(h, plan_grown_cap(0, most, 256)));
    }
    std::vector<size_t> at((size_t)nb + 1, 0);
    for (int k = 0; k < nb; k++) at[k + 1] = at[k] + (max_pairs > 0 ? (size_t)cnt[2 * k] : 0);
    got.resize(at[nb]);
    for (int k = 0; k < nb; k++)
        if (at[k + 1] > at[k])
            HIP_TRY(hc.copy(got.data() + at[k], h->map.dup.list + (size_t)(b0 + k) * h->map.dup.cap, sizeof(ekf_dup_pair) * (at[k + 1] - at[k]), hipMemcpyDeviceToHost));
    if (at[nb] > 0) HIP_TRY(hc.wait());
    for (int k = 0; k < nb; k++) {
        const int found = cnt[2 * k];
        if (n_found_out) n_found_out[k] = found;
        if (n_degenerate_out) n_degenerate_out[k] = cnt[2 * k + 1];
        if (at[k + 1] == at[k]) continue;
        std::sort(got.begin() + at[k], got.begin() + at[k + 1], [](const ekf_dup_pair &a, const ekf_dup_pair &b) { return a.i != b.i ? a.i < b.i : a.j < b.j; });
        memcpy(pairs_out + (size_t)k * max_pairs, got.data() + at[k], sizeof(ekf_dup_pair) * (size_t)(found < max_pairs ? found : max_pairs));
    }
    return nb == 1 && !n_found_out ? cnt[0] : EKF_OK;
}

static bool dup_args_ok(double gate, double max_dist, const ekf_dup_pair *pairs_out, int max_pairs) {
    return __builtin_isfinite(gate) && gate >= 0.0 && max_dist == max_dist && max_pairs >= 0 && (pairs_out || max_pairs == 0);
}

extern "C" int ekf_find_duplicates(ekf_handle h, int index, double gate, double max_dist, int split, ekf_dup_pair *pairs_out, int max_pairs,
                                   int *n_degenerate_out) {
    if (!filter_ok(h, index) || split < 0 || !dup_args_ok(gate, max_dist, pairs_out, max_pairs)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return dup_impl(h, filters_of(h, index), gate, max_dist, split, nullptr, pairs_out, max_pairs, nullptr, n_degenerate_out);
}

extern "C" int ekf_batch_find_duplicates(ekf_handle h, double gate, double max_dist, const int *split, ekf_dup_pair *pairs_out, int max_pairs, int *n_found_out,
                                         int *n_degenerate_out) {
    if (!h || !n_found_out || !dup_args_ok(gate, max_dist, pairs_out, max_pairs)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return dup_impl(h, filters_of(h, -1), gate, max_dist, 0, split, pairs_out, max_pairs, n_found_out, n_degenerate_out);
}

// ---- the rounds of the fusion machinery -----------------------------------------------------------
// What every client's call does around its own kernels (ekf_fuse.hip), on a settled handle with FuseScratch built and the client's
// tables queued: the progress record of the filters f cleared; per round of at most ekf_window() of the longest list's `most`
// entries the client's front(round, m_hi) -- m_hi the most entries of a filter in the round; n_max the most landmarks of a filter
// of the call, the caller's --, which ends with its factor's fuse_publish and W's landmark rows in the FA slot rows, then k_fuse_apply, k_fuse_finish
// and one dense pass over set 0, in place in the settled buffer in either pipeline mode (also on handles whose chain kernel folds
// its own windows); last the progress record's copy to done [nb][2], queued on *hc: the caller waits.
// n_max == 0 -- a position or heading fix where no filter of the call has a landmark; a fused pair or a matched measurement names
// a landmark of its filter, so for those clients the guards never fail -- would make the gather, k_fuse_apply and the pass launches
// of zero blocks: the round is the factor and k_fuse_finish (P_RR and the pose) alone.
template <typename Front>
static int fuse_rounds(ekf_batch *h, Filters f, int most, int n_max, HostCopies *hc, int *done, Front front) {
    const EkfDev &dv = h->dv;
    const FuseScratch fs = h->map.fuse;
    hipStream_t s = h->s_chain;
    const int b0 = f.b0, nb = f.nb, nT = lm_tiles(n_max);
    HIP_TRY(hipMemsetAsync(fs.done + 2 * (size_t)b0, 0, sizeof(int) * 2 * (size_t)nb, s));
    HIP_TRY(hipMemsetAsync(fs.m_round + b0, 0, sizeof(int) * (size_t)nb, s));
    for (int round = 0; round * dv.maxp < most; round++) {
        front(round, std::min(most - round * dv.maxp, dv.maxp));
        if (n_max > 0) hipLaunchKernelGGL(k_fuse_apply, dim3((unsigned)cdiv(64 * nT, 256), (unsigned)nb), dim3(256), 0, s, dv, fs, b0);
        hipLaunchKernelGGL(k_fuse_finish, dim3((unsigned)nb), dim3(64), 0, s, dv, fs, b0);
        if (n_max > 0) launch_pass(dv, s, nullptr, nullptr, /*interleave*/ false, nT, /*set*/ 0, dv.maxp, h->win.buf_in, h->win.buf_in, nullptr, /*rev*/ 0, b0, nb);
    }
    HIP_TRY(hc->copy(done, fs.done + 2 * (size_t)b0, sizeof(int) * 2 * (size_t)nb, hipMemcpyDeviceToHost));
    return EKF_OK;
}

// ---- landmark fusion ------------------------------------------------------------------------------
// The filters f, filter f.b0 + k with n_pairs[k] pairs at pairs + k * ld_pairs.  The list is checked against the mirror's
// landmark counts before anything else happens to the handle; a call without a pair returns there.  Then: settle, the pair table
// up, the rounds (fuse_rounds: the gather, then the factor), the progress record back, and the removal of the fused pairs' j
// through remove_settled, which ends the rewrite.  Nothing fused anywhere: the rewrite is ended here (slot rows cleared, the pass
// sizes restored).
static int fuse_impl(ekf_batch *h, Filters f, const ekf_dup_pair *pairs, int ld_pairs, const int *n_pairs, double slack, int *n_fused_out, int *n_lm_out) {
    const int b0 = f.b0, nb = f.nb;
    // the one way out: n_lm[k] landmarks in filter b0 + k now, done[2 k] of its pairs fused (done == nullptr: none anywhere)
    const auto leave = [=](const int *n_lm, const int *done) {
        for (int k = 0; k < nb; k++) {
            if (n_fused_out) n_fused_out[k] = done ? done[2 * k] : 0;
            if (n_lm_out) n_lm_out[k] = n_lm[k];
        }
        return nb == 1 && !n_lm_out ? n_lm[0] : EKF_OK;
    };
    HIP_TRY(hipSetDevice(h->device));
    EKF_TRY(refresh_bounds(h, false));
    int most;
    EKF_TRY(set_error(plan_fuse_pairs(pairs, ld_pairs, n_pairs, counts_of(h, b0), b0, nb, &most)));
    if (most == 0) return leave(counts_of(h, b0), nullptr);  // nothing to do: the window stays open
    // h_int[b] = landmarks of filter b; a sticky EKF_ERR_TIMEOUT or EKF_ERR_CAPACITY ends it here: the state stays as it is; then
    // every deferred slot folded, both streams idle
    EKF_TRY(quiesce(h, QUIET_SETTLED, ST_INVALID_OR_FULL));
    EKF_TRY(fuse_reserve(h));
    EkfDev &dv = h->dv;
    const FuseScratch fs = h->map.fuse;
    hipStream_t s = h->s_chain;
    const int n_max = most_landmarks(counts_of(h, b0), nb);
    std::vector<int> tab, done((size_t)2 * nb, 0);
    EKF_TRY(set_error(plan_fuse_table(pairs, ld_pairs, n_pairs, nb, fs.pcap, &tab)));
    HostCopies hc(s);
    HIP_TRY(hc.copy(fs.pairs + (size_t)b0 * fs.pcap * 2, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hc.copy(fs.cnt + b0, n_pairs, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice));
    // the gather runs BEFORE the factor: S is taken from the gathered rows (a fused pair names two landmarks: n_max > 0)
    EKF_TRY(fuse_rounds(h, f, most, n_max, &hc, done.data(), [&](int round, int m_hi) {
        hipLaunchKernelGGL(k_fuse_gather, dim3((unsigned)cdiv(n_max, 256), (unsigned)m_hi, (unsigned)nb), dim3(256), 0, s, dv, fs, h->win.buf_in, round, b0);
        hipLaunchKernelGGL(k_fuse_factor, dim3((unsigned)nb), dim3(256), 0, s, dv, fs, round, slack, b0);
    }));
    HIP_TRY(hc.wait());
    EKF_TRY(check_launch());
    // the fused pairs' j go, exactly as ekf_remove_landmarks with keep[j] = 0 removes them
    const int ld_keep = n_max > 0 ? n_max : 1;
    std::vector<unsigned char> keep((size_t)nb * ld_keep, 1);
    bool any = false;
    for (int k = 0; k < nb; k++) {
        if (n_fused_out) n_fused_out[k] = done[2 * k];  // (filled even where the removal below fails)
        for (int q = 0; q < done[2 * k]; q++) keep[(size_t)k * ld_keep + pairs[(size_t)k * ld_pairs + q].j] = 0;
        any = any || done[2 * k] > 0;
    }
    std::vector<int> n_new(counts_of(h, b0), counts_of(h, b0) + nb);
    if (any) EKF_TRY(remove_settled(h, f, keep.data(), ld_keep, n_new.data()));
    else EKF_TRY(finish_rewrite(h, b0, nb, /*rearm*/ true, n_new.data(), 1, /*flip_buf*/ false));
    return leave(n_new.data(), done.data());
}

extern "C" int ekf_fuse_landmarks(ekf_handle h, int index, const ekf_dup_pair *pairs, int n_pairs, double slack, int *n_fused_out) {
    if (!filter_ok(h, index) || n_pairs < 0 || (n_pairs > 0 && !pairs) || !(__builtin_isfinite(slack) && slack >= 0.0))
        return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return fuse_impl(h, filters_of(h, index), pairs, n_pairs, &n_pairs, slack, n_fused_out, nullptr);
}

extern "C" int ekf_batch_fuse_landmarks(ekf_handle h, const ekf_dup_pair *pairs, int ld_pairs, const int *n_pairs, double slack, int *n_fused_out,
                                        int *n_landmarks_out) {
    if (!h || !n_pairs || ld_pairs < 0 || !n_landmarks_out || !(__builtin_isfinite(slack) && slack >= 0.0)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return fuse_impl(h, filters_of(h, -1), pairs, ld_pairs, n_pairs, slack, n_fused_out, n_landmarks_out);
}

// ---- list updates: matched measurements and absolute fixes -----------------------------------------
// The call's lists into the scratch of filters [b0, b0 + nb), through the caller's guard (the host tables live until it has waited).
static int match_upload(ekf_batch *h, const MatchTable &t, int b0, int nb, HostCopies *hc) {
    const MatchScratch &ms = h->map.match;
    const size_t at = (size_t)b0 * ms.zcap, cnt = (size_t)nb * ms.zcap;
    HIP_TRY(hc->copy(ms.z + 2 * at, t.zt.data(), sizeof(double) * 2 * cnt, hipMemcpyHostToDevice));
    HIP_TRY(hc->copy(ms.Rm + 4 * at, t.Rt.data(), sizeof(double) * 4 * cnt, hipMemcpyHostToDevice));
    HIP_TRY(hc->copy(ms.ids + at, t.idt.data(), sizeof(int) * cnt, hipMemcpyHostToDevice));
    HIP_TRY(hc->copy(ms.cnt + b0, t.cnt.data(), sizeof(int) * (size_t)nb, hipMemcpyHostToDevice));
    return EKF_OK;
}

// d2 of the device's lists back into the caller's order: entry q of filter k, if it is one of its first n_valid[2 k], to
// d2_out[k * n_z + src]; everything else NaN.  n_valid == nullptr: every entry.
static void match_scatter(const MatchTable &t, const std::vector<double> &d2, int zcap, int n_z, int nb, const int *n_valid, double *d2_out) {
    if (!d2_out) return;
    for (size_t q = 0; q < (size_t)nb * n_z; q++) d2_out[q] = __builtin_nan("");
    for (int k = 0; k < nb; k++) {
        const int cnt = n_valid ? n_valid[2 * k] : t.cnt[k];
        for (int q = 0; q < cnt; q++) d2_out[(size_t)k * n_z + t.src[(size_t)k * zcap + q]] = d2[(size_t)k * zcap + q];
    }
}

// The iterations of ekf_update_matched_iter (ekf_match_iter.hip) and where their per-measurement results go; a list update without
// one linearises once, by its client's own factor.
struct IterArgs {
    int max_iter;
    double tol;
    int *iters_out;    // [nb][n] or null
    double *step_out;  // [nb][n] or null
};
// The iterations' results in the caller's order, as match_scatter places d2: 0 and NaN for the skipped and the unapplied entries.
static void iter_scatter(const MatchTable &t, const std::vector<int> &iters, const std::vector<double> &step, int tcap, int icap, int n_z, int nb, const int *n_valid,
                         const IterArgs &it) {
    for (size_t q = 0; q < (size_t)nb * n_z; q++) {
        if (it.iters_out) it.iters_out[q] = 0;
        if (it.step_out) it.step_out[q] = __builtin_nan("");
    }
    for (int k = 0; k < nb; k++)
        for (int q = 0; q < n_valid[2 * k]; q++) {
            const size_t to = (size_t)k * n_z + t.src[(size_t)k * tcap + q];
            if (it.iters_out) it.iters_out[to] = iters[(size_t)k * icap + q];
            if (it.step_out) it.step_out[to] = step[(size_t)k * icap + q];
        }
}

// A list client of the fusion machinery: the checks and the tables of its lists (ekf_map_plan.h) and its two kernels.
struct ListClient {
    PlanStatus (*values)(const double *z, const double *R, const int *ids, int n, int b0, int nb, int limit);
    PlanStatus (*ids)(const int *ids, int n, const int *n_lm, int b0, int nb, int *most);
    MatchTable (*table)(const double *z, const double *R, const int *ids, int n, int nb, int zcap);
    void (*factor)(EkfDev dv, FuseScratch fs, MatchScratch ms, int buf, int round, int rs, int apply, int b_off);
    void (*gather)(EkfDev dv, FuseScratch fs, MatchScratch ms, int buf, int round, int b_off);
};
static const ListClient MATCHED = {plan_match_values, plan_match_ids, plan_match_table, k_match_factor, k_match_gather};  // ekf_match.hip
static const ListClient FIXES = {plan_fix_values, plan_fix_ids, plan_fix_table, k_fix_factor, k_fix_gather};              // ekf_fix.hip; ids carries the kinds
// ekf_polar.hip; ids is the packed list of polar_front: the landmark with its kind above it
static const ListClient POLAR = {plan_polar_values, plan_polar_ids, plan_polar_table, k_polar_factor, k_polar_gather};

// The filters f, filter f.b0 + k with the n entries at z + k * n * 2, R + k * n * 4, ids + k * n.  The values are checked before
// anything happens to the handle, the ids against the mirror's landmark counts; a call without an entry returns there.  Then:
// settle, the tables up, the rounds (fuse_rounds: the client's factor, then its gather), the progress record and the distances back
// in one copy each, and the end of the rewrite (slot rows cleared, the pass sizes restored, the mirror's pose and P_RR refreshed by
// k_set_meta).  With `it` (the MATCHED client alone) the round's factor is k_match_factor_iter, and the factorisations and the last
// step of every entry come back with the distances.
static int list_update_impl(const ListClient &c, ekf_batch *h, Filters f, const double *z, const double *R, const int *ids, int n, int *n_applied_out, double *d2_out,
                            const IterArgs *it = nullptr) {
    const int b0 = f.b0, nb = f.nb;
    EKF_TRY(set_error(c.values(z, R, ids, n, b0, nb, -1)));
    HIP_TRY(hipSetDevice(h->device));
    EKF_TRY(refresh_bounds(h, false));
    int most;
    EKF_TRY(set_error(c.ids(ids, n, counts_of(h, b0), b0, nb, &most)));
    if (most == 0) {  // nothing to do: the window stays open
        for (int k = 0; n_applied_out && k < nb; k++) n_applied_out[k] = 0;
        for (size_t q = 0; d2_out && q < (size_t)nb * n; q++) d2_out[q] = __builtin_nan("");
        if (it) iter_scatter({}, {}, {}, 0, 0, n > 0 ? n : 0, nb, std::vector<int>((size_t)2 * nb, 0).data(), *it);
        return nb == 1 ? h->h_int[b0] : EKF_OK;
    }
    // h_int[b] = landmarks of filter b; a sticky EKF_ERR_TIMEOUT or EKF_ERR_CAPACITY ends it here: the state stays as it is; then
    // every deferred slot folded, both streams idle
    EKF_TRY(quiesce(h, QUIET_SETTLED, ST_INVALID_OR_FULL));
    EKF_TRY(fuse_reserve(h));
    EKF_TRY(match_reserve(h, most));
    if (it) EKF_TRY(iter_reserve(h, most));
    const EkfDev &dv = h->dv;
    const FuseScratch fs = h->map.fuse;
    const MatchScratch ms = h->map.match;
    const IterScratch is = h->map.iter;
    hipStream_t s = h->s_chain;
    const MatchTable tab = c.table(z, R, ids, n, nb, ms.zcap);
    std::vector<int> done((size_t)2 * nb, 0), iters(it ? (size_t)nb * is.zcap : 0);
    std::vector<double> d2((size_t)nb * ms.zcap), step(iters.size());
    HostCopies hc(s);
    EKF_TRY(match_upload(h, tab, b0, nb, &hc));
    const int n_max = most_landmarks(counts_of(h, b0), nb);
    // The factor runs BEFORE the gather: a filter whose S is refused gathers nothing.
    EKF_TRY(fuse_rounds(h, f, most, n_max, &hc, done.data(), [&](int round, int m_hi) {
        if (it) hipLaunchKernelGGL(k_match_factor_iter, dim3((unsigned)nb), dim3(256), 0, s, dv, fs, ms, is, h->win.buf_in, round, dv.maxp, it->max_iter, it->tol, b0);
        else hipLaunchKernelGGL(c.factor, dim3((unsigned)nb), dim3(256), 0, s, dv, fs, ms, h->win.buf_in, round, dv.maxp, /*apply*/ 1, b0);
        if (n_max > 0) hipLaunchKernelGGL(c.gather, dim3((unsigned)cdiv(n_max, 256), (unsigned)m_hi, (unsigned)nb), dim3(256), 0, s, dv, fs, ms, h->win.buf_in, round, b0);
    }));
    HIP_TRY(hc.copy(d2.data(), ms.d2 + (size_t)b0 * ms.zcap, sizeof(double) * d2.size(), hipMemcpyDeviceToHost));
    if (it) {
        HIP_TRY(hc.copy(iters.data(), is.iters + (size_t)b0 * is.zcap, sizeof(int) * iters.size(), hipMemcpyDeviceToHost));
        HIP_TRY(hc.copy(step.data(), is.step + (size_t)b0 * is.zcap, sizeof(double) * step.size(), hipMemcpyDeviceToHost));
    }
    HIP_TRY(hc.wait());
    EKF_TRY(check_launch());
    for (int k = 0; n_applied_out && k < nb; k++) n_applied_out[k] = done[2 * k];  // (filled even where the end of the rewrite fails)
    match_scatter(tab, d2, ms.zcap, n, nb, done.data(), d2_out);
    if (it) iter_scatter(tab, iters, step, ms.zcap, is.zcap, n, nb, done.data(), *it);
    const std::vector<int> n_lm(counts_of(h, b0), counts_of(h, b0) + nb);
    EKF_TRY(finish_rewrite(h, b0, nb, /*rearm*/ true, n_lm.data(), 1, /*flip_buf*/ false));
    return nb == 1 ? n_lm[0] : EKF_OK;
}

// The score alone: the rule of ekf_get_state (the streaming launch leaves, every deferred slot is folded, both streams idle), then
// the settled state is only read: the tables up, the client's factor with apply = 0 over one round of up to EKF_MAX_PENDING, d2 back.
static int list_compat_impl(const ListClient &c, ekf_batch *h, Filters f, const double *z, const double *R, const int *ids, int n, double *d2_out) {
    const int b0 = f.b0, nb = f.nb;
    if (!d2_out && n > 0) return set_error(EKF_ERR_BAD_ARG, "d2_out is null");
    EKF_TRY(set_error(c.values(z, R, ids, n, b0, nb, EKF_MAX_PENDING)));
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_INVALID));
    int most;
    EKF_TRY(set_error(c.ids(ids, n, counts_of(h, b0), b0, nb, &most)));
    for (size_t q = 0; q < (size_t)nb * (n > 0 ? n : 0); q++) d2_out[q] = __builtin_nan("");
    if (most == 0) return EKF_OK;  // (nothing is folded)
    EKF_TRY(settle(h));
    EKF_TRY(match_reserve(h, most));
    const MatchScratch ms = h->map.match;
    hipStream_t s = h->s_chain;
    const MatchTable tab = c.table(z, R, ids, n, nb, ms.zcap);
    std::vector<double> d2((size_t)nb * ms.zcap);
    HostCopies hc(s);
    EKF_TRY(match_upload(h, tab, b0, nb, &hc));
    hipLaunchKernelGGL(c.factor, dim3((unsigned)nb), dim3(256), 0, s, h->dv, h->map.fuse, ms, h->win.buf_in, 0, EKF_MAX_PENDING, /*apply*/ 0, b0);
    HIP_TRY(hc.copy(d2.data(), ms.d2 + (size_t)b0 * ms.zcap, sizeof(double) * d2.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hc.wait());
    EKF_TRY(check_launch());
    match_scatter(tab, d2, ms.zcap, n, nb, nullptr, d2_out);
    return EKF_OK;
}

extern "C" int ekf_update_matched(ekf_handle h, int index, const double *z, const double *R, const int *ids, int n_z, int *n_applied_out, double *d2_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return list_update_impl(MATCHED, h, filters_of(h, index), z, R, ids, n_z, n_applied_out, d2_out);
}

extern "C" int ekf_batch_update_matched(ekf_handle h, const double *z, const double *R, const int *ids, int n_z, int *n_applied_out, double *d2_out) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    const int rc = list_update_impl(MATCHED, h, filters_of(h, -1), z, R, ids, n_z, n_applied_out, d2_out);
    return rc < 0 ? rc : EKF_OK;
}

extern "C" int ekf_update_matched_iter(ekf_handle h, int index, const double *z, const double *R, const int *ids, int n_z, int max_iter, double tol, int *n_applied_out,
                                       double *d2_out, int *iters_out, double *step_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    EKF_TRY(set_error(plan_iter_args(max_iter, tol)));
    const IterArgs it = {max_iter, tol, iters_out, step_out};
    return list_update_impl(MATCHED, h, filters_of(h, index), z, R, ids, n_z, n_applied_out, d2_out, &it);
}

extern "C" int ekf_batch_update_matched_iter(ekf_handle h, const double *z, const double *R, const int *ids, int n_z, int max_iter, double tol, int *n_applied_out,
                                             double *d2_out, int *iters_out, double *step_out) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    EKF_TRY(set_error(plan_iter_args(max_iter, tol)));
    const IterArgs it = {max_iter, tol, iters_out, step_out};
    const int rc = list_update_impl(MATCHED, h, filters_of(h, -1), z, R, ids, n_z, n_applied_out, d2_out, &it);
    return rc < 0 ? rc : EKF_OK;
}

extern "C" int ekf_joint_compat(ekf_handle h, int index, const double *z, const double *R, const int *ids, int n_z, double *d2_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return list_compat_impl(MATCHED, h, filters_of(h, index), z, R, ids, n_z, d2_out);
}

extern "C" int ekf_batch_joint_compat(ekf_handle h, const double *z, const double *R, const int *ids, int n_z, double *d2_out) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    return list_compat_impl(MATCHED, h, filters_of(h, -1), z, R, ids, n_z, d2_out);
}

extern "C" int ekf_update_fixes(ekf_handle h, int index, const double *z, const double *R, const int *what, int n, int *n_applied_out, double *d2_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return list_update_impl(FIXES, h, filters_of(h, index), z, R, what, n, n_applied_out, d2_out);
}

extern "C" int ekf_batch_update_fixes(ekf_handle h, const double *z, const double *R, const int *what, int n, int *n_applied_out, double *d2_out) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    const int rc = list_update_impl(FIXES, h, filters_of(h, -1), z, R, what, n, n_applied_out, d2_out);
    return rc < 0 ? rc : EKF_OK;
}

extern "C" int ekf_fix_compat(ekf_handle h, int index, const double *z, const double *R, const int *what, int n, double *d2_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return list_compat_impl(FIXES, h, filters_of(h, index), z, R, what, n, d2_out);
}

extern "C" int ekf_batch_fix_compat(ekf_handle h, const double *z, const double *R, const int *what, int n, double *d2_out) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    return list_compat_impl(FIXES, h, filters_of(h, -1), z, R, what, n, d2_out);
}

// The polar calls' front: the caller's ids and kinds into the one list a ListClient takes (plan_polar_pack: its checks run here,
// before the handle is touched, the POLAR client's own behind them), then the update or, with apply == 0, the score.
static int polar_front(ekf_batch *h, Filters f, const double *z, const double *R, const int *ids, const int *kind, int n, int *n_applied_out, double *d2_out, int apply) {
    std::vector<int> packed;
    EKF_TRY(set_error(plan_polar_pack(ids, kind, n, f.b0, f.nb, &packed)));
    const int *p = n > 0 ? packed.data() : nullptr;
    return apply ? list_update_impl(POLAR, h, f, z, R, p, n, n_applied_out, d2_out) : list_compat_impl(POLAR, h, f, z, R, p, n, d2_out);
}

extern "C" int ekf_update_polar(ekf_handle h, int index, const double *z, const double *R, const int *ids, const int *kind, int n, int *n_applied_out, double *d2_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return polar_front(h, filters_of(h, index), z, R, ids, kind, n, n_applied_out, d2_out, /*apply*/ 1);
}

extern "C" int ekf_batch_update_polar(ekf_handle h, const double *z, const double *R, const int *ids, const int *kind, int n, int *n_applied_out, double *d2_out) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    const int rc = polar_front(h, filters_of(h, -1), z, R, ids, kind, n, n_applied_out, d2_out, /*apply*/ 1);
    return rc < 0 ? rc : EKF_OK;
}

extern "C" int ekf_polar_compat(ekf_handle h, int index, const double *z, const double *R, const int *ids, const int *kind, int n, double *d2_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return polar_front(h, filters_of(h, index), z, R, ids, kind, n, nullptr, d2_out, /*apply*/ 0);
}

extern "C" int ekf_batch_polar_compat(ekf_handle h, const double *z, const double *R, const int *ids, const int *kind, int n, double *d2_out) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    return polar_front(h, filters_of(h, -1), z, R, ids, kind, n, nullptr, d2_out, /*apply*/ 0);
}

// ---- individual compatibility ---------------------------------------------------------------------
// The filters f, filter f.b0 + k with the n_z measurements at z + k * n_z * 2 and R + k * n_z * 4 (valid + k * n_z masks them).  The
// values are checked before anything happens to the handle; a call without a measurement returns there.  Then the rule of
// ekf_get_landmark_covs: the chain stream idle (a resident streaming launch leaves first), NOTHING folded -- x, the robot rows and D
// are current inside an open window --, the flush stream untouched.  The tables up, the two kernels, the counters and the
// per-measurement results back, then the lists.  A call that finds more than the device list holds and has to hand some out runs
// the kernels once more with a list that fits (the state has not moved: the same pairs).  The appended order is the hardware's;
// each filter's list is sorted here (plan_gate_sort).  Returns `found` of the one filter when n_found_out is null.
static int gate_impl(ekf_batch *h, Filters f, const double *z, const double *R, const unsigned char *valid, int n_z, double gate, ekf_candidate *cand_out, int max_cand,
                     int *n_found_out, ekf_decision *nearest_out, int *n_skipped_out) {
    const int b0 = f.b0, nb = f.nb;
    EKF_TRY(set_error(plan_gate_args(z, R, valid, n_z, b0, nb, gate, cand_out, max_cand)));
    for (int k = 0; n_found_out && k < nb; k++) n_found_out[k] = 0;
    if (n_z == 0) return EKF_OK;
    const int most = plan_gate_most(valid, n_z, nb);
    HIP_TRY(hipSetDevice(h->device));
    EKF_TRY(refresh_bounds(h));  // the chain stream idle; h_int[b] = landmarks of filter b; a sticky EKF_ERR_TIMEOUT ends it here
    if (most == 0) {  // every entry masked
        plan_gate_scatter(plan_gate_table(z, R, valid, n_z, nb, 1), 1, n_z, nb, nullptr, nullptr, nearest_out, n_skipped_out);
        return EKF_OK;
    }
    EKF_TRY(gate_reserve(h, most, max_cand > 0 ? list_cap_for(max_cand) : 0));
    const EkfDev &dv = h->dv;
    hipStream_t s = h->s_chain;
    const int zcap = h->map.gate.zcap, n_max = most_landmarks(counts_of(h, b0), nb);
    const GateTable tab = plan_gate_table(z, R, valid, n_z, nb, zcap);
    const size_t at0 = (size_t)b0 * zcap, nent = (size_t)nb * zcap;
    std::vector<int> cnt((size_t)nb, 0), skip(nent);
    std::vector<ekf_decision> near(nent);
    std::vector<ekf_candidate> got;
    HostCopies hc(s);
    HIP_TRY(hc.copy(h->map.gate.z + 2 * at0, tab.zt.data(), sizeof(double) * 2 * nent, hipMemcpyHostToDevice));
    HIP_TRY(hc.copy(h->map.gate.Rm + 4 * at0, tab.Rt.data(), sizeof(double) * 4 * nent, hipMemcpyHostToDevice));
    HIP_TRY(hc.copy(h->map.gate.nz + b0, tab.cnt.data(), sizeof(int) * (size_t)nb, hipMemcpyHostToDevice));
    for (int round = 0;; round++) {
        const GateScratch gs = h->map.gate;
        HIP_TRY(hipMemsetAsync(gs.cnt + b0, 0, sizeof(int) * (size_t)nb, s));
        if (n_max > 0) hipLaunchKernelGGL(k_gate, dim3((unsigned)cdiv(n_max, GATE_THREADS), (unsigned)nb), dim3(GATE_THREADS), 0, s, dv, gs, gate, b0);
        if (round == 0) hipLaunchKernelGGL(k_gate_nearest, dim3((unsigned)cdiv(most, 64), (unsigned)nb), dim3(64), 0, s, dv, gs, b0);
        HIP_TRY(hc.copy(cnt.data(), gs.cnt + b0, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost));
        if (round == 0) {
            HIP_TRY(hc.copy(near.data(), gs.near + at0, sizeof(ekf_decision) * nent, hipMemcpyDeviceToHost));
            HIP_TRY(hc.copy(skip.data(), gs.skip + at0, sizeof(int) * nent, hipMemcpyDeviceToHost));
        }
        HIP_TRY(hc.wait());
        EKF_TRY(check_launch());
        const int most_found = most_landmarks(cnt.data(), nb);
        if (most_found <= gs.ccap || max_cand == 0) break;
        if (round > 0) return set_error(EKF_ERR_STATE, "the candidate count changed between two passes over an unchanged state");
        EKF_TRY(gate_reserve(h, most, plan_grown_cap(0, most_found, 256)));
    }
    // the lists back in ONE copy, a row of the longest list per filter (what lies behind a filter's own count is not looked at)
    const size_t row = max_cand > 0 ? (size_t)most_landmarks(cnt.data(), nb) : 0;
    got.resize((size_t)nb * row);
    if (row > 0) {
        HIP_TRY(hc.copy2d(got.data(), row * sizeof(ekf_candidate), h->map.gate.list + (size_t)b0 * h->map.gate.ccap, (size_t)h->map.gate.ccap * sizeof(ekf_candidate),
                          row * sizeof(ekf_candidate), (size_t)nb, hipMemcpyDeviceToHost));
        HIP_TRY(hc.wait());
    }
    for (int k = 0; k < nb; k++) {
        if (n_found_out) n_found_out[k] = cnt[k];
        if (row == 0 || cnt[k] == 0) continue;
        ekf_candidate *mine = got.data() + (size_t)k * row;
        if (!plan_gate_sort(mine, (size_t)cnt[k], tab.src.data() + (size_t)k * zcap, tab.cnt[k])) return set_error(EKF_ERR_STATE, "a listed candidate names no measurement of the call");
        memcpy(cand_out + (size_t)k * max_cand, mine, sizeof(ekf_candidate) * (size_t)(cnt[k] < max_cand ? cnt[k] : max_cand));
    }
    plan_gate_scatter(tab, zcap, n_z, nb, near.data(), skip.data(), nearest_out, n_skipped_out);
    return n_found_out ? EKF_OK : cnt[0];
}

extern "C" int ekf_gate_candidates(ekf_handle h, int index, const double *z, const double *R, int n_z, double gate, ekf_candidate *cand_out, int max_cand,
                                   ekf_decision *nearest_out, int *n_skipped_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return gate_impl(h, filters_of(h, index), z, R, nullptr, n_z, gate, cand_out, max_cand, nullptr, nearest_out, n_skipped_out);
}

extern "C" int ekf_batch_gate_candidates(ekf_handle h, const double *z, const double *R, const unsigned char *valid, int n_z, double gate, ekf_candidate *cand_out,
                                         int max_cand, int *n_found_out, ekf_decision *nearest_out, int *n_skipped_out) {
    if (!h || !n_found_out) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return gate_impl(h, filters_of(h, -1), z, R, valid, n_z, gate, cand_out, max_cand, n_found_out, nearest_out, n_skipped_out);
}

// ---- joint compatibility search -------------------------------------------------------------------
extern "C" int ekf_joint_gates(double confidence, double *out) {
    if (!out || !plan_assoc_gates(confidence, out)) return set_error(EKF_ERR_BAD_ARG, "bad argument (a confidence inside (0, 1))");
    return EKF_OK;
}

// The filters f with the scans of gate_impl.  The values are checked before anything happens to the handle.  Then the rule of
// ekf_joint_compat: the streaming launch leaves, a sticky EKF_ERR_TIMEOUT ends the call; the sweep of ekf_gate_candidates (gate_impl
// itself, nothing folded: its list comes back sorted, and GateScratch keeps the compacted measurements on the device); the
// per-measurement table from the list (plan_assoc_table: this is the one trip through the host, the sort gate_impl makes anyway --
// a second sweep only when a filter lists more than 2 048 pairs).  No candidate anywhere: returns, nothing folded.  Else settle(),
// the table up, k_assoc_search (one launch: one wave per filter), k_match_factor with apply = 0 on the winner it left in
// MatchScratch -- ekf_joint_compat's kernel, so d2_out has ekf_joint_compat's bits --, the results back in three copies.
static int assoc_impl(ekf_batch *h, Filters f, const double *z, const double *R, const unsigned char *valid, int n_z, double gate, const double *joint_gate, int max_branch,
                      long long max_nodes, int *ids_out, double *d2_out, ekf_decision *nearest_out, int *n_skipped_out, ekf_assoc *info_out) {
    const int b0 = f.b0, nb = f.nb;
    EKF_TRY(set_error(plan_assoc_args(z, R, valid, n_z, b0, nb, gate, joint_gate, max_branch, max_nodes, ids_out, EKF_MAX_PENDING)));
    AssocArgs aa;
    if (joint_gate) memcpy(aa.jg, joint_gate, sizeof aa.jg);
    else plan_assoc_gates(0.99, aa.jg);
    aa.max_nodes = max_nodes;
    EKF_TRY(quiesce(h, QUIET_STREAM, ST_INVALID));
    std::vector<int> found((size_t)nb, 0);
    std::vector<ekf_candidate> cands;
    size_t ld = 0;
    if (n_z > 0) {
        const size_t all = (size_t)n_z * (size_t)(h->dv.Ncap > 0 ? h->dv.Ncap : 1);  // (a filter cannot list more)
        ld = all < 2048 ? all : 2048;
        for (int round = 0;; round++) {
            cands.resize((size_t)nb * ld);
            const int rc = gate_impl(h, f, z, R, valid, n_z, gate, cands.data(), (int)ld, found.data(), nearest_out, n_skipped_out);
            if (rc < 0) return rc;
            const size_t most = (size_t)most_landmarks(found.data(), nb);
            if (most <= ld) break;
            if (round > 0) return set_error(EKF_ERR_STATE, "the candidate count changed between two passes over an unchanged state");
            ld = most;
        }
    }
    const AssocTable tab = plan_assoc_table(cands.data(), ld, found.data(), valid, n_z, nb, max_branch);
    std::vector<ekf_assoc> info((size_t)nb);
    for (int k = 0; k < nb; k++) info[k] = ekf_assoc{0, 0.0, 0, 1, tab.listed[k], tab.dropped[k]};
    std::vector<int> ids;
    std::vector<double> d2;
    size_t ld_d2 = 0;
    if (tab.any) {
        EKF_TRY(settle(h));
        EKF_TRY(assoc_reserve(h));
        EKF_TRY(match_reserve(h, EKF_MAX_PENDING));
        const AssocScratch as = h->map.assoc;
        const MatchScratch ms = h->map.match;
        hipStream_t s = h->s_chain;
        const size_t per = EKF_MAX_PENDING;
        std::vector<AssocResult> out((size_t)nb);
        ids.resize((size_t)nb * per), d2.resize((size_t)nb * ms.zcap), ld_d2 = (size_t)ms.zcap;
        HostCopies hc(s);
        HIP_TRY(hc.copy(as.ncand + b0 * per, tab.ncand.data(), sizeof(int) * nb * per, hipMemcpyHostToDevice));
        HIP_TRY(hc.copy(as.cand + b0 * per * EKF_ASSOC_MAX_BRANCH, tab.cand.data(), sizeof(int) * nb * per * EKF_ASSOC_MAX_BRANCH, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_assoc_search, dim3((unsigned)nb), dim3(64), 0, s, h->dv, h->map.gate, as, ms, aa, h->win.buf_in, b0);
        hipLaunchKernelGGL(k_match_factor, dim3((unsigned)nb), dim3(256), 0, s, h->dv, h->map.fuse, ms, h->win.buf_in, 0, EKF_MAX_PENDING, /*apply*/ 0, b0);
        HIP_TRY(hc.copy(ids.data(), as.ids + b0 * per, sizeof(int) * nb * per, hipMemcpyDeviceToHost));
        HIP_TRY(hc.copy(out.data(), as.out + b0, sizeof(AssocResult) * (size_t)nb, hipMemcpyDeviceToHost));
        HIP_TRY(hc.copy(d2.data(), ms.d2 + (size_t)b0 * ms.zcap, sizeof(double) * d2.size(), hipMemcpyDeviceToHost));
        HIP_TRY(hc.wait());
        EKF_TRY(check_launch());
        for (int k = 0; k < nb; k++) info[k].nodes = out[k].nodes, info[k].d2 = out[k].d2, info[k].n_paired = out[k].n_paired, info[k].complete = out[k].complete;
    }
    if (n_z > 0) plan_assoc_scatter(tab, tab.any ? ids.data() : nullptr, d2.data(), ld_d2, n_z, nb, ids_out, d2_out);
    for (int k = 0; info_out && k < nb; k++) info_out[k] = info[k];
    return nb == 1 ? info[0].n_paired : EKF_OK;
}

extern "C" int ekf_associate_joint(ekf_handle h, int index, const double *z, const double *R, int n_z, double gate, const double *joint_gate, int max_branch, long long max_nodes,
                                   int *ids_out, double *d2_out, ekf_decision *nearest_out, int *n_skipped_out, ekf_assoc *info_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return assoc_impl(h, filters_of(h, index), z, R, nullptr, n_z, gate, joint_gate, max_branch, max_nodes, ids_out, d2_out, nearest_out, n_skipped_out, info_out);
}

extern "C" int ekf_batch_associate_joint(ekf_handle h, const double *z, const double *R, const unsigned char *valid, int n_z, double gate, const double *joint_gate,
                                         int max_branch, long long max_nodes, int *ids_out, double *d2_out, ekf_decision *nearest_out, int *n_skipped_out,
                                         ekf_assoc *info_out) {
    if (!h || !info_out) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    const int rc = assoc_impl(h, filters_of(h, -1), z, R, valid, n_z, gate, joint_gate, max_branch, max_nodes, ids_out, d2_out, nearest_out, n_skipped_out, info_out);
    return rc < 0 ? rc : EKF_OK;
}

// ---- landmark initialisation ----------------------------------------------------------------------
// The filters f, filter f.b0 + k with the n_z measurements at z + k * n_z * 2 and R + k * n_z * 4, of which add + k * n_z selects
// (the caller has run plan_add_args).  Nothing selected anywhere: the counts from the mirror, the window stays open.  Else the
// join's order: settle, the room (one filter without it ends the call: not sticky, nothing has run), the table up in one copy, the
// three kernels on the chain stream (ekf_rewrite.hip), in place in the settled buffer in either pipeline mode, and the end of the
// rewrite.  ids_out [nb][n_z] (may be null), n_out [nb].
static int add_impl(ekf_batch *h, Filters f, const double *z, const double *R, const unsigned char *add, int n_z, int *ids_out, int *n_out) {
    const int b0 = f.b0, nb = f.nb;
    const int most = plan_gate_most(add, n_z, nb);
    HIP_TRY(hipSetDevice(h->device));
    if (most == 0) {  // nothing to do: the window stays open
        EKF_TRY(refresh_bounds(h, false));
        for (size_t q = 0; ids_out && q < (size_t)nb * (n_z > 0 ? n_z : 0); q++) ids_out[q] = -1;
        for (int k = 0; k < nb; k++) n_out[k] = h->h_int[b0 + k];
        return EKF_OK;
    }
    // h_int[b] = landmarks of filter b; a sticky EKF_ERR_TIMEOUT or EKF_ERR_CAPACITY ends it here: the state stays as it is; then
    // every deferred slot folded, both streams idle
    EKF_TRY(quiesce(h, QUIET_SETTLED, ST_INVALID_OR_FULL));
    EkfDev &dv = h->dv;
    const int zcap = plan_add_zcap(h->map.add.zcap, most);
    const AddTable tab = plan_add_table(z, R, add, n_z, nb, zcap);
    EKF_TRY(set_error(plan_add_room(counts_of(h, b0), tab.cnt.data(), b0, nb, dv.Ncap, "add")));
    EKF_TRY(add_reserve(h, most));
    const AddScratch as = h->map.add;
    std::vector<int> ids((size_t)nb * (n_z > 0 ? n_z : 0)), n_new((size_t)nb);
    int nt, m_hi;
    plan_add_ids(tab, counts_of(h, b0), n_z, nb, zcap, ids.data(), n_new.data(), &nt, &m_hi);
    hipStream_t s = h->s_chain;
    HostCopies hc(s);
    HIP_TRY(hc.copy(as.tab + (size_t)b0 * add_tab_stride(zcap), tab.tab.data(), sizeof(double) * tab.tab.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_add_vec, dim3((unsigned)cdiv(m_hi, 64), (unsigned)nb), dim3(64), 0, s, dv, as, b0);
    if (nt > 0) hipLaunchKernelGGL(k_add_tiles, dim3((unsigned)nt, (unsigned)nb), dim3(256), 0, s, dv, h->win.buf_in, as, b0);
    hipLaunchKernelGGL(k_add_finish, dim3((unsigned)nb), dim3(64), 0, s, dv, as, b0);
    EKF_TRY(finish_rewrite(h, b0, nb, /*rearm*/ true, nullptr, 0, /*flip_buf*/ false));
    hc.waited();
    if (ids_out && !ids.empty()) memcpy(ids_out, ids.data(), sizeof(int) * ids.size());
    for (int k = 0; k < nb; k++) n_out[k] = n_new[k];
    return EKF_OK;
}

extern "C" int ekf_add_landmarks(ekf_handle h, int index, const double *z, const double *R, const unsigned char *add, int n_z, int *ids_out) {
    if (!h || index < 0) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    EKF_TRY(set_error(plan_add_args(z, R, add, n_z, index, h->dv.B, nullptr)));
    int n;
    EKF_TRY(add_impl(h, filters_of(h, index), z, R, add, n_z, ids_out, &n));
    return n;
}

extern "C" int ekf_batch_add_landmarks(ekf_handle h, const double *z, const double *R, const unsigned char *add, int n_z, int *ids_out, int *n_out) {
    if (!h) return set_error(EKF_ERR_BAD_ARG, "null handle");
    EKF_TRY(set_error(plan_add_args(z, R, add, n_z, -1, h->dv.B, n_out)));
    return add_impl(h, filters_of(h, -1), z, R, add, n_z, ids_out, n_out);
}

// ---- the scan step --------------------------------------------------------------------------------
// ekf_associate_joint, ekf_update_matched and ekf_add_landmarks of one scan as one call: assoc_impl at the entry state (ids and the
// filter's own gate per measurement), the kinds (plan_joint_kinds), the room for the New ones -- nothing has been applied yet --,
// list_update_impl (MATCHED) with the pairings, add_impl with the New ones at the state the matched step left.  Every step is the public call's own
// implementation with the public call's arguments: the same bits.
static int update_joint_impl(ekf_batch *h, Filters f, const double *z, const double *R, const unsigned char *valid, int n_z, double gate, const double *joint_gate,
                             int max_branch, long long max_nodes, int *ids_out, int *kind_out, double *d2_out, ekf_assoc *info_out, int *n_out) {
    const int b0 = f.b0, nb = f.nb;
    const size_t all = (size_t)nb * (n_z > 0 ? n_z : 0);
    std::vector<ekf_decision> near(all);
    int rc = assoc_impl(h, f, z, R, valid, n_z, gate, joint_gate, max_branch, max_nodes, ids_out, nullptr, near.data(), nullptr, info_out);
    if (rc < 0) return rc;
    std::vector<int> kind(all), n_add((size_t)nb, 0), applied((size_t)nb, 0), new_ids(all, -1);
    std::vector<unsigned char> is_new(all);
    plan_joint_kinds(ids_out, near.data(), valid, n_z, nb, kind.data(), is_new.data());
    for (int k = 0; k < nb; k++)
        for (int q = 0; q < n_z; q++) n_add[k] += is_new[(size_t)k * n_z + q];
    EKF_TRY(set_error(plan_add_room(counts_of(h, b0), n_add.data(), b0, nb, h->dv.Ncap, "update")));  // (assoc_impl has refreshed the counts)
    rc = list_update_impl(MATCHED, h, f, z, R, ids_out, n_z, applied.data(), d2_out);
    if (rc < 0) return rc;
    rc = add_impl(h, f, z, R, is_new.data(), n_z, new_ids.data(), n_out);
    if (rc < 0) return rc;
    plan_joint_merge(applied.data(), new_ids.data(), n_z, nb, ids_out, kind.data());
    if (kind_out && all) memcpy(kind_out, kind.data(), sizeof(int) * all);
    return EKF_OK;
}

extern "C" int ekf_update_joint(ekf_handle h, int index, const double *z, const double *R, int n_z, double gate, const double *joint_gate, int max_branch,
                                long long max_nodes, int *ids_out, int *kind_out, double *d2_out, ekf_assoc *info_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    int n;
    EKF_TRY(update_joint_impl(h, filters_of(h, index), z, R, nullptr, n_z, gate, joint_gate, max_branch, max_nodes, ids_out, kind_out, d2_out, info_out, &n));
    return n;
}

extern "C" int ekf_batch_update_joint(ekf_handle h, const double *z, const double *R, const unsigned char *valid, int n_z, double gate, const double *joint_gate,
                                      int max_branch, long long max_nodes, int *ids_out, int *kind_out, double *d2_out, ekf_assoc *info_out, int *n_out) {
    if (!h || !info_out || !n_out) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return update_joint_impl(h, filters_of(h, -1), z, R, valid, n_z, gate, joint_gate, max_branch, max_nodes, ids_out, kind_out, d2_out, info_out, n_out);
}

// ---- relocalisation -------------------------------------------------------------------------------
// The filters f, filter f.b0 + k with the n_z measurements at z + k * n_z * 2 (valid + k * n_z masks them).  The values are checked
// before anything happens to the handle.  Then the rule of ekf_gate_candidates: the chain stream idle (a resident streaming launch
// leaves first), NOTHING folded -- x is current inside an open window --, the flush stream untouched.  A call in which no filter has
// a base pair and two landmarks returns there, without scratch.  The tables up (plan_locate_table), k_loc_pairs and the counts
// back; a filter beyond EKF_LOCATE_MAX_CAND ends the call (not sticky, the state was only read); a list that does not hold what
// was found is replaced and the pairs run once more (the state has not moved: the same candidates).  Then the score, the two
// selection stages and the fit with nothing in between, the records and the ids back in one copy each, the compacted measurement
// indices turned into the caller's.  hyp_out [nb][max_out], ids_out [nb][max_out][n_z], n_found [nb] = the hypotheses written.
static int locate_impl(ekf_batch *h, Filters f, const double *z, const unsigned char *valid, int n_z, double tol, double min_sep, int max_base, int max_out,
                       ekf_locate_hyp *hyp_out, int *ids_out, int *n_found, long long *n_cand_out) {
    const int b0 = f.b0, nb = f.nb;
    EKF_TRY(set_error(plan_locate_args(z, valid, n_z, b0, nb, tol, min_sep, max_base, max_out, hyp_out, ids_out, EKF_MAX_PENDING)));
    for (int k = 0; k < nb; k++) {
        n_found[k] = 0;
        if (n_cand_out) n_cand_out[k] = 0;
    }
    HIP_TRY(hipSetDevice(h->device));
    EKF_TRY(refresh_bounds(h));  // the chain stream idle; h_int[b] = landmarks of filter b; a sticky EKF_ERR_TIMEOUT ends it here
    LocateTable tab = plan_locate_table(z, valid, n_z, nb, min_sep, max_base);
    bool any = false;
    for (int k = 0; k < nb; k++) {
        if (counts_of(h, b0)[k] < 2) tab.nbase[k] = 0;
        any = any || tab.nbase[k] > 0;
    }
    if (!any) return EKF_OK;  // (no scratch either)
    EKF_TRY(loc_reserve(h, LOC_LIST_FLOOR));
    const EkfDev &dv = h->dv;
    hipStream_t s = h->s_chain;
    const int n_max = most_landmarks(counts_of(h, b0), nb), most = most_landmarks(tab.cnt.data(), nb);
    const size_t per = EKF_MAX_PENDING, bcap = EKF_LOCATE_MAX_BASE, ocap = EKF_LOCATE_MAX_OUT;
    std::vector<unsigned long long> cnt((size_t)nb, 0);
    std::vector<ekf_locate_hyp> hyps((size_t)nb * ocap);
    std::vector<int> ids((size_t)nb * ocap * per);
    HostCopies hc(s);
    {
        const LocScratch &ls = h->map.loc;
        HIP_TRY(hc.copy(ls.z + b0 * per * 2, tab.zt.data(), sizeof(double) * nb * per * 2, hipMemcpyHostToDevice));
        HIP_TRY(hc.copy(ls.blen + b0 * bcap, tab.blen.data(), sizeof(double) * nb * bcap, hipMemcpyHostToDevice));
        HIP_TRY(hc.copy(ls.base + b0 * bcap * 2, tab.base.data(), sizeof(int) * nb * bcap * 2, hipMemcpyHostToDevice));
        HIP_TRY(hc.copy(ls.nz + b0, tab.cnt.data(), sizeof(int) * (size_t)nb, hipMemcpyHostToDevice));
        HIP_TRY(hc.copy(ls.nbase + b0, tab.nbase.data(), sizeof(int) * (size_t)nb, hipMemcpyHostToDevice));
    }
    unsigned long long most_found = 0;
    for (int round = 0;; round++) {
        const LocScratch ls = h->map.loc;
        const unsigned side = (unsigned)cdiv(n_max, LOC_THREADS);
        HIP_TRY(hipMemsetAsync(ls.cnt + b0, 0, sizeof(unsigned long long) * (size_t)nb, s));
        hipLaunchKernelGGL(k_loc_pairs, dim3(side, side, (unsigned)nb), dim3(LOC_THREADS), 0, s, dv, ls, 2.0 * tol, b0);
        HIP_TRY(hc.copy(cnt.data(), ls.cnt + b0, sizeof(unsigned long long) * (size_t)nb, hipMemcpyDeviceToHost));
        HIP_TRY(hc.wait());
        EKF_TRY(check_launch());
        most_found = *std::max_element(cnt.begin(), cnt.end());
        for (int k = 0; n_cand_out && k < nb; k++) n_cand_out[k] = (long long)cnt[k];
        for (int k = 0; k < nb; k++)
            if (cnt[k] > (unsigned long long)EKF_LOCATE_MAX_CAND)
                return set_error(EKF_ERR_CAPACITY, "filter %d: %llu candidates, more than EKF_LOCATE_MAX_CAND = %d: tol too loose for this map", b0 + k, cnt[k], EKF_LOCATE_MAX_CAND);
        if (most_found <= (unsigned long long)ls.ccap) break;
        if (round > 0) return set_error(EKF_ERR_STATE, "the candidate count changed between two passes over an unchanged state");
        EKF_TRY(loc_reserve(h, plan_grown_cap(0, (long long)most_found, LOC_LIST_FLOOR)));
    }
    if (most_found > 0) {
        const LocScratch ls = h->map.loc;
        const int groups = cdiv((int)most_found, LOC_THREADS / 64), parts = std::min(LOC_PICK_PARTS, cdiv((int)most_found, 4096));
        const dim3 gs((unsigned)std::min(groups, 2048), (unsigned)nb);
        const auto k_score = most <= 8 ? k_loc_score<8> : most <= 16 ? k_loc_score<16> : k_loc_score<EKF_MAX_PENDING>;
        hipLaunchKernelGGL(k_score, gs, dim3(LOC_THREADS), 0, s, dv, ls, tol * tol, b0);
        hipLaunchKernelGGL(k_loc_pick, dim3((unsigned)parts, (unsigned)nb), dim3(LOC_THREADS), 0, s, ls, 0, max_out, b0);
        hipLaunchKernelGGL(k_loc_pick, dim3(1, (unsigned)nb), dim3(LOC_THREADS), 0, s, ls, 1, max_out, b0);
        hipLaunchKernelGGL(k_loc_fit, dim3((unsigned)std::min<unsigned long long>(most_found, (unsigned long long)max_out), (unsigned)nb), dim3(64), 0, s, dv, ls, tol * tol, b0);
        HIP_TRY(hc.copy(hyps.data(), ls.hyp + b0 * ocap, sizeof(ekf_locate_hyp) * hyps.size(), hipMemcpyDeviceToHost));
        HIP_TRY(hc.copy(ids.data(), ls.ids + b0 * ocap * per, sizeof(int) * ids.size(), hipMemcpyDeviceToHost));
        HIP_TRY(hc.wait());
        EKF_TRY(check_launch());
    }
    for (int k = 0; k < nb; k++) {
        const int written = (int)std::min<unsigned long long>(cnt[k], (unsigned long long)max_out);
        const int *src = tab.src.data() + (size_t)k * per;
        n_found[k] = written;
        for (int t = 0; t < written; t++) {
            ekf_locate_hyp hy = hyps[(size_t)k * ocap + t];
            if (hy.meas_a < 0 || hy.meas_a >= tab.cnt[k] || hy.meas_b < 0 || hy.meas_b >= tab.cnt[k]) return set_error(EKF_ERR_STATE, "a hypothesis names no measurement of the call");
            hy.meas_a = src[hy.meas_a], hy.meas_b = src[hy.meas_b];
            hyp_out[(size_t)k * max_out + t] = hy;
            int *row = ids_out + ((size_t)k * max_out + t) * n_z;
            for (int q = 0; q < n_z; q++) row[q] = -1;
            for (int q = 0; q < tab.cnt[k]; q++) row[src[q]] = ids[((size_t)k * ocap + t) * per + q];
        }
    }
    return EKF_OK;
}

extern "C" int ekf_locate_scan(ekf_handle h, int index, const double *z, int n_z, double tol, double min_sep, int max_base, int max_out, ekf_locate_hyp *hyp_out, int *ids_out,
                               long long *n_cand_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    int found = 0;
    EKF_TRY(locate_impl(h, filters_of(h, index), z, nullptr, n_z, tol, min_sep, max_base, max_out, hyp_out, ids_out, &found, n_cand_out));
    return found;
}

extern "C" int ekf_batch_locate_scan(ekf_handle h, const double *z, const unsigned char *valid, int n_z, double tol, double min_sep, int max_base, int max_out,
                                     ekf_locate_hyp *hyp_out, int *ids_out, int *n_found_out, long long *n_cand_out) {
    if (!h || !n_found_out) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return locate_impl(h, filters_of(h, -1), z, valid, n_z, tol, min_sep, max_base, max_out, hyp_out, ids_out, n_found_out, n_cand_out);
}

// The pose reset on the device (ekf_rewrite.hip: k_reset_pose), the order of steps as in reframe_impl: settle, one launch over the
// robot rows, the end of the rewrite (slot rows cleared).  pose [nb][3], prr [nb][9] (checked by the caller: plan_reset_args);
// apply [nb] or null: the filters to reset.  A one-filter call carries its argument in the kernel arguments, the batch form in a
// transient table (104 bytes per filter).
static int reset_impl(ekf_batch *h, Filters f, const double *pose, const double *prr, const unsigned char *apply) {
    // h_int[b] = landmarks of filter b; a sticky EKF_ERR_TIMEOUT or EKF_ERR_CAPACITY ends it here: the state stays as it is; then
    // every deferred slot folded, both streams idle
    EKF_TRY(quiesce(h, QUIET_SETTLED, ST_INVALID_OR_FULL));
    const int b0 = f.b0, nb = f.nb, n_max = most_landmarks(counts_of(h, b0), nb);
    std::vector<double> vals((size_t)nb * 13);
    for (int k = 0; k < nb; k++) plan_reset_values(pose + 3 * (size_t)k, prr + 9 * (size_t)k, !apply || apply[k], vals.data() + 13 * (size_t)k);
    DevTmp<double> tab_d;
    ResetPose one;
    EKF_TRY(rewrite_arg(vals, nb, &one, &tab_d));
    hipLaunchKernelGGL(k_reset_pose, dim3((unsigned)cdiv(3 + 2 * n_max, 256), (unsigned)nb), dim3(256), 0, h->s_chain, h->dv, one, (const double *)tab_d.p, b0);
    return finish_rewrite(h, b0, nb, /*rearm*/ true, nullptr, 0, /*flip_buf*/ false);
}

extern "C" int ekf_reset_pose(ekf_handle h, int index, const double pose[3], const double P_RR[9]) {
    if (!filter_ok(h, index) || !pose) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    EKF_TRY(set_error(plan_reset_args(pose, P_RR, index)));
    return reset_impl(h, filters_of(h, index), pose, P_RR, nullptr);
}

extern "C" int ekf_batch_reset_pose(ekf_handle h, const double *pose, const double *P_RR) {
    if (!h || !pose || !P_RR) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    for (int b = 0; b < h->dv.B; b++) EKF_TRY(set_error(plan_reset_args(pose + 3 * (size_t)b, P_RR + 9 * (size_t)b, b)));
    return reset_impl(h, filters_of(h, -1), pose, P_RR, nullptr);
}

// ekf_locate_scan, the acceptance rule, ekf_reset_pose and ekf_update_matched of one scan as one call: every step is the public
// call's own implementation with the public call's arguments -- the same bits.  Everything the later steps would refuse for their
// values (R, P_RR) is refused before the search.  No filter accepted: returns behind the search, which only reads.  hyp_out [nb],
// ids_out [nb][n_z], d2_out [nb][n_z] (may be null), n_out [nb] = the best hypothesis's inliers, or 0: refused.
static int relocalize_impl(ekf_batch *h, Filters f, const double *z, const double *R, const unsigned char *valid, int n_z, double tol, double min_sep, int max_base,
                           int max_out, int min_inliers, int lead, const double *prr, ekf_locate_hyp *hyp_out, int *ids_out, double *d2_out, int *n_out) {
    const int b0 = f.b0, nb = f.nb;
    if (!hyp_out || !ids_out || !prr || min_inliers < 2 || lead < 0 || n_z < 0 || (n_z > 0 && (!z || !R)) || max_out < 1 || max_out > EKF_LOCATE_MAX_OUT)
        return set_error(EKF_ERR_BAD_ARG, "bad argument (min_inliers >= 2, lead >= 0, max_out in 1 .. %d, no null list)", EKF_LOCATE_MAX_OUT);
    for (int k = 0; k < nb; k++) {
        EKF_TRY(set_error(plan_reset_args(nullptr, prr + 9 * (size_t)k, b0 + k)));
        for (int q = 0; q < n_z; q++) {
            const size_t at = (size_t)k * n_z + q;
            if ((!valid || valid[at]) && !(__builtin_isfinite(z[2 * at]) && __builtin_isfinite(z[2 * at + 1]) && plan_entry_finite(z, R, at)))
                return set_error(EKF_ERR_BAD_ARG, "filter %d, measurement %d: z or R is not finite", b0 + k, q);
        }
    }
    const size_t all = (size_t)nb * n_z;
    std::vector<ekf_locate_hyp> hyps((size_t)nb * max_out);
    std::vector<int> ids((size_t)nb * max_out * (n_z > 0 ? n_z : 1)), found((size_t)nb, 0);
    EKF_TRY(locate_impl(h, f, z, valid, n_z, tol, min_sep, max_base, max_out, hyps.data(), ids.data(), found.data(), nullptr));
    const LocateTable tab = plan_locate_table(z, valid, n_z, nb, min_sep, 1);  // (its reach)
    std::vector<unsigned char> accepted((size_t)nb, 0);
    std::vector<double> poses((size_t)nb * 3, 0.0);
    std::vector<int> ids_m(all > 0 ? all : 1, -1);
    bool any = false;
    for (int k = 0; k < nb; k++) {
        const ekf_locate_hyp *mine = hyps.data() + (size_t)k * max_out;
        accepted[k] = plan_locate_accept(mine, found[k], tol, tab.reach[k], min_inliers, lead);
        any = any || accepted[k];
        n_out[k] = accepted[k] ? mine[0].inliers : 0;
        if (found[k] > 0) hyp_out[k] = mine[0];
        else memset(&hyp_out[k], 0, sizeof(ekf_locate_hyp));
        for (int q = 0; q < n_z; q++) ids_out[(size_t)k * n_z + q] = found[k] > 0 ? ids[(size_t)k * max_out * n_z + q] : -1;
        for (int q = 0; q < n_z; q++) ids_m[(size_t)k * n_z + q] = accepted[k] ? ids_out[(size_t)k * n_z + q] : -1;
        for (int i = 0; i < 3; i++) poses[3 * (size_t)k + i] = accepted[k] ? mine[0].pose[i] : 0.0;
    }
    for (size_t q = 0; d2_out && q < all; q++) d2_out[q] = __builtin_nan("");
    if (!any) return EKF_OK;
    EKF_TRY(reset_impl(h, f, poses.data(), prr, nb == 1 ? nullptr : accepted.data()));
    std::vector<int> applied((size_t)nb, 0);
    const int rc = list_update_impl(MATCHED, h, f, z, R, ids_m.data(), n_z, applied.data(), d2_out);
    return rc < 0 ? rc : EKF_OK;
}

extern "C" int ekf_relocalize(ekf_handle h, int index, const double *z, const double *R, int n_z, double tol, double min_sep, int max_base, int max_out, int min_inliers,
                              int lead, const double P_RR[9], ekf_locate_hyp *hyp_out, int *ids_out, double *d2_out) {
    if (!filter_ok(h, index)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    int n = 0;
    EKF_TRY(relocalize_impl(h, filters_of(h, index), z, R, nullptr, n_z, tol, min_sep, max_base, max_out, min_inliers, lead, P_RR, hyp_out, ids_out, d2_out, &n));
    return n;
}

extern "C" int ekf_batch_relocalize(ekf_handle h, const double *z, const double *R, const unsigned char *valid, int n_z, double tol, double min_sep, int max_base,
                                    int max_out, int min_inliers, int lead, const double *P_RR, ekf_locate_hyp *hyp_out, int *ids_out, double *d2_out, int *n_out) {
    if (!h || !n_out) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    return relocalize_impl(h, filters_of(h, -1), z, R, valid, n_z, tol, min_sep, max_base, max_out, min_inliers, lead, P_RR, hyp_out, ids_out, d2_out, n_out);
}

extern "C" int ekf_get_landmark_covs(ekf_handle h, int index, double *cov_out, int n_max) {
    if (!filter_ok(h, index) || n_max < 0 || (!cov_out && n_max > 0)) return set_error(EKF_ERR_BAD_ARG, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    EKF_TRY(refresh_bounds(h));  // the chain stream idle (a resident streaming launch leaves first); no pass, the flush stream untouched
    const int N = h->h_int[index];
    const int cnt = N < n_max ? N : n_max;
    if (cnt == 0) return N;
    std::vector<double> comp((size_t)3 * cnt);  // the three components of the always-current diagonal blocks
    HostCopies hc(h->s_chain);
    HIP_TRY(hc.copy2d(comp.data(), (size_t)cnt * sizeof(double), h->dv.D + (size_t)index * 3 * h->dv.dn, (size_t)h->dv.dn * sizeof(double), (size_t)cnt * sizeof(double), 3,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hc.wait());
    for (int l = 0; l < cnt; l++)
        for (int c = 0; c < 3; c++) cov_out[3 * l + c] = comp[(size_t)c * cnt + l];
    return N;
}
