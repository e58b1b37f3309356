// nf_capi_field.hip -- the C ABI of libnemoflux_amd.so, part 3 of 3: Level 2, the Field-shaped engine (field.py:15-234;
// BASELINE north_star's computeFlux(tIndex)): nf_field_*.  Host-side orchestration only: every number is produced by the HIP
// kernels of nf_geom.hip / nf_flux.hip / nf_weights.hip / nf_integral.hip.  There is no CPU path.
#include "nf_capi.h"

using namespace nf;

// 1 = compute_all may put all time steps of a small grid into one launch per kernel ("batch_steps" tuning knob)
static int g_batch_steps = 1;
// nf_tuning_set knobs of this file (the library reads no environment variable):
//   "batch_cellsteps_m"    the all-steps-in-one-launch form is used while nt*ncell stays under this many Mi cell-steps (32)
//   "partial_step_planes"  1 = a rank's PARTIAL time steps keep the six-plane epilogue (the code before round 4: the before
//                          leg of profiles/r04_rank_emulation.txt); 0 = signed planes only (default)
//   "graph"                0 = nf_field_compute_all_async never replays a captured graph of the pass (default 1)
//   "pass_inner_signed"    1 = inside one per-step pass, every owned step but the last stores only the two signed planes
//                          (K3 reads nothing else and the next step overwrites all six); 0 = every step stores what it
//                          stores on its own (default 1)
//   "pass_k3_pairs"        1 = the per-step pass reduces its whole steps two at a time: one gather launch reads the record
//                          stream once for both steps; 0 = one reduction per step (default 1)
//   "pass_inner_interleaved"  1 = the steps of a pair whose planes no caller can read -- the first step of every pair, and the
//                          second of every pair but the pass's last -- store ONE interleaved (eU, eV) stream, which the pair
//                          reduction gathers with three loads per record instead of four; 0 = two planes each, the pass as it
//                          was without the form; -1 = by the dtype of uo / vo, as measured (default: see g_inner_interleaved)
//   "class_window"         rows of the class transport per pass over the fields, 1 .. 32 (default 32: DESIGN.md section 4)
//   "area_chunk"           levels per launch of the area profile: 2 or 4 (float64), 4 or 8 (float32); 0 = the measured default
//   "gross_chunk"          levels per launch of the gross profile: 2, 4 or 8 (float64), 4 or 8 (float32); 0 = the measured default
//   "crossing_chunk"       levels per launch of the crossings: 2, 4 or 8; 0 = the measured default of the form (the same bits either way)
//   "joint_window"         rows of the joint class transport (and of the gross class transport and the class area) per pass
//                          over the term table, 1 .. 32 (default 32)
//   "joint_skip"           1 = a block of the joint binning whose records have no term in the window does not read the table
//                          (default 1: docs/EXPERIMENTS.md); the rows are the same bits either way
static long g_batch_cellsteps = 32l << 20;
static int g_partial_full = 0;
static int g_use_graph = 1;
static int g_inner_signed = 1;
static int g_k3_pairs = 1;
// Measured in-process at the headline size (tools/ab_pass.py, profiles/pass_interleaved.txt): float64 -1.2 % per pass, the
// ranges of nine rounds apart; float32 +0.6 % -- there the flux kernel's four 16-byte stores at a 64-byte lane stride cost it
// more (+2.8 % per launch) than the reduction gains.  So the default (-1) interleaves float64 passes only.
static int g_inner_interleaved = -1;
static int g_class_window = 32;
static int g_joint_window = 32;
static int g_joint_skip = 1;
static long g_knob_version = 0;   // bumped by every knob of this file: a captured pass bakes them in

namespace nf {
int field_tuning_set(const char *name, int value)
{
    ++g_knob_version;
    if (!strcmp(name, "batch_steps")) {
        g_batch_steps = value;
        return NF_OK;
    }
    if (!strcmp(name, "batch_cellsteps_m")) {
        if (!(value >= 0 && value <= 2047)) return -1;   // nf_tuning_set then reports the knob as unknown / out of range
        g_batch_cellsteps = (long)value << 20;
        return NF_OK;
    }
    if (!strcmp(name, "partial_step_planes")) {
        g_partial_full = value != 0;
        return NF_OK;
    }
    if (!strcmp(name, "graph")) {
        g_use_graph = value != 0;
        return NF_OK;
    }
    if (!strcmp(name, "pass_inner_signed")) {
        g_inner_signed = value != 0;
        return NF_OK;
    }
    if (!strcmp(name, "pass_k3_pairs")) {
        g_k3_pairs = value != 0;
        return NF_OK;
    }
    if (!strcmp(name, "pass_inner_interleaved")) {
        if (!(value >= -1 && value <= 1)) return -1;
        g_inner_interleaved = value;
        return NF_OK;
    }
    if (!strcmp(name, "class_window")) {
        if (!(value >= 1 && value <= kClassWindowMax)) return -1;
        g_class_window = value;
        return NF_OK;
    }
    if (!strcmp(name, "joint_window")) {
        if (!(value >= 1 && value <= kClassWindowMax)) return -1;
        g_joint_window = value;
        return NF_OK;
    }
    if (!strcmp(name, "joint_skip")) {
        if (!(value == 0 || value == 1)) return -1;
        g_joint_skip = value;
        return NF_OK;
    }
    if (!strcmp(name, "area_chunk")) return area_chunk_set(value);
    if (!strcmp(name, "gross_chunk")) return gross_chunk_set(value);
    if (!strcmp(name, "crossing_chunk")) return crossing_chunk_set(value);
    return -1;
}
}  // namespace nf

// =============================================================================================== Level 2
// One input series of a Field: an (nt, nz, ny, nx) array of the dtype of uo / vo that lives in HBM or on the host (a file-backed
// one arrives as a host array, one step at a time), or a pair that differs only in the pointer: uo / vo, e3u / e3v.  A tracer
// uses p[0] and stage[0] alone.
struct Series {
    const void *p[2] = {nullptr, nullptr};
    long nt = 0;
    int dtype = NF_F64, on_device = 1;
    double fill = std::numeric_limits<double>::quiet_NaN();
    double fill2 = std::numeric_limits<double>::quiet_NaN();   // the second marker (missing_value)
    // host-resident arrays: the owned levels of one step (field_stage).  Sized with the element size of uo / vo for every
    // series; they only grow and survive a re-set of their series.
    DevArray<char> stage[2];
};

// Class edges on the host, uploaded by the next compute after a change
struct EdgeSet {
    std::vector<double> host;
    bool stale = false;
    DevArray<double> dev;   // `cap` doubles
    int upload(size_t cap, hipStream_t s)
    {
        if (!stale) return NF_OK;
        // the host copy may change again before an asynchronous copy from pageable memory has read it: wait for this one
        NF_TRY(dev.reserve(cap));
        NF_HIP(hipMemcpyAsync(dev.get(), host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, s));
        NF_HIP(hipStreamSynchronize(s));
        stale = false;
        return NF_OK;
    }
};

struct nf_field {
    hipStream_t stream = nullptr;
    long ny = 0, nx = 0, ncell = 0, nz = 0;
    // everything sized by the grid: allocated by set_bounds (and on demand after it), dropped together by field_free_geometry
    struct Geometry {
        DevArray<double> xy, arc4, arcE, arcN;
        DevArray<unsigned long long> box;
        // resident per-step outputs
        DevArray<double> iV;    // [4][ncell]
        DevArray<double> abs;   // [2][ncell]
        DevArray<double> aos;   // (ncell,4) re-pack buffer for read_step, allocated on first use
        // the steps of a pair that do not go to the resident planes ("pass_k3_pairs"), 2 * ncell doubles each, allocated on
        // first use: pair[0] the first step's [eU | eV] planes or ("pass_inner_interleaved") its interleaved stream; pair[1]
        // the interleaved stream of the second step of a pair that is not the pass's last
        DevArray<double> pair[2];
        DevArray<double> tr_planes;   // [2][ncell] eU_tau, eV_tau of the last tracer step, allocated on first use
        DevArray<unsigned long long> maxbits;
        // multi-step launches for small grids (compute_all): per-step planes, scratch and z ranges
        DevArray<double> iVb, absb, scratchb;
        DevArray<int> zr;
        long batch_steps = 0, batch_version = -1;
    } geo;
    double box[4] = {0, 0, 0, 0};
    DevArray<double> thick;
    // velocity fields uo / vo (nf_field_set_uv, nf_field_set_missing_value): their nt and dtype are the Field's
    Series uv;
    int sverdrup = 0;
    long s_begin = 0, s_end = -1;
    // compact resident mode (nf_field_set_compact): the flux kernel stores only eU and eV; the neighbour-copy planes and
    // the two |.| planes are derived when somebody asks for them (read_step, device_ptr)
    int compact = 0;
    bool derived_stale = false;
    // transects
    std::vector<std::vector<double>> polylines;
    std::vector<int> poly_cc;
    std::vector<int> tr_off;
    WeightSet ws;
    bool weights_built = false;
    int skip_unsupported = 0;   // nf_field_set_unsupported_cells
    int overlap_warn = 0;       // nf_field_set_overlapping_cells
    DevArray<int> tr_off_dev;
    DevArray<double> scratch;   // the run sums of two steps (a pair of the per-step pass)
    // depth-resolved rows (nf_field_compute_profile): the run sums of one chunk of levels (ws.nrec * kProfileChunk, allocated
    // on first use, dropped with the weights)
    DevArray<double> prof_scratch;
    DevArray<double> row;   // the result of a synchronous call (field_sync): a row, or the (nz, row_length) block of a profile
    // tracer at T-points (nf_field_set_tracer*): same (nt, nz, ny, nx) and dtype as uo / vo; none of its setters changes
    // `version`, and nothing of it enters a captured pass
    Series tau;
    double tau_ref = 0.0;
    int tau_wrap = 1;
    // class tracer at T-points (nf_field_set_class_tracer*): the field whose classes the class calls bin by; nullptr: the
    // tracer above.  No reference; the wrap rule is the tracer's.  Its setters change neither `version` nor a captured pass.
    Series sig;
    // per-cell layer thicknesses (nf_field_set_cell_thickness): e3u / e3v of (e3.nt, nz, ny, nx), e3.nt == 1 (static) or nt, in
    // the dtype of uo / vo; nullptr: the per-level thickness above.  A static host array is uploaded once into e3?_static
    // and counts as resident from then on; a time-varying host array is staged per step, owned levels only.  Setting or
    // clearing them changes `version`.
    Series e3;
    DevArray<char> e3u_static, e3v_static;
    // the (nz, ny, nx) in force when e3?_static were uploaded: the upload belongs to that shape (field_cell_thick_current)
    long e3_static_nz = 0, e3_static_ny = 0, e3_static_nx = 0;
    // tracer profile (nf_field_compute_tracer_profile): the run sums of one chunk (ws.nrec * tracer_profile_chunk(dtype))
    DevArray<double> tprof_scratch;
    // area profile (nf_field_compute_area_profile): the run sums of one chunk, two values per level (ws.nrec * 2 * area_chunk)
    DevArray<double> area_scratch;
    // gross profile (nf_field_compute_gross_profile): the run sums of one chunk, two values per level (ws.nrec * 2 * gross_chunk)
    DevArray<double> gross_scratch;
    // crossings (nf_field_compute_crossings): the planes of a synchronous call, (2 or 4) * nz * ws.nrec doubles, sized on demand
    // as `row` is and dropped with the weights
    DevArray<double> crossings;
    // class transport (nf_field_set_class_edges): the edges; the run sums of one window of rows (ws.nrec * window, allocated on
    // first use, dropped with the weights)
    EdgeSet class_edges;
    DevArray<double> class_scratch;
    // transports in depth bins (nf_field_set_depth_edges): edges of their own and the depth of the upper interface of level 0;
    // the run sums of a window go to class_scratch
    EdgeSet depth_edges;
    double depth_top = 0.0;
    // transports between surfaces (nf_field_set_depth_surfaces): m 2-D fields of (nt, ny, nx), nt == 1 (static) or the nt of
    // uo / vo, in their dtype; a state of its own that no other product reads.  HBM arrays are used in place, a static host set
    // is uploaded once into `fixed` (m planes) and counts as resident from then on, a time-varying host set is staged one
    // step at a time into `stage`.  Its setters change neither `version` nor a captured pass.
    struct Surfaces {
        const void *p[kMaxSurfaces] = {};
        int m = 0;
        long nt = 0;
        int dtype = NF_F64, on_device = 1;
        double fill = std::numeric_limits<double>::quiet_NaN();
        double fill2 = std::numeric_limits<double>::quiet_NaN();
        int wrap = 1;
        double top = 0.0;
        DevArray<char> fixed, stage;
        long fixed_ny = 0, fixed_nx = 0;   // the (ny, nx) in force when `fixed` was uploaded (field_surfaces_current)
    } surf;
    // joint class transport (nf_field_set_joint_class_edges): state of its own, the 1-D forms do not see it.  The edges of
    // axis A then axis B in one set.  The term table (40 bytes per record and
    // owned level), the block flags and the run sums of one window are allocated on first use, grown when the records, the
    // owned levels or the rows ask for more -- their layout is taken from the call's own sizes, never from an earlier one's
    // -- and dropped with the weights.  The gross class transport (nf_field_compute_gross_class_transport) and the class area
    // (nf_field_compute_class_area, two table entries per record and owned level) use the same three buffers with the 1-D
    // class edges: each call sizes them for itself.
    EdgeSet joint_edges;
    int joint_na = 0, joint_nb = 0;
    DevArray<char> joint_table;
    DevArray<unsigned> joint_flags;
    DevArray<double> joint_scratch;
    Grid_t grid_view;
    // timing
    bool timing = false;
    struct TimedLaunch {         // events around one flux launch (+ expansion); mid sits between the two kernels;
        hipEvent_t e0 = nullptr, mid = nullptr, e1 = nullptr, e2 = nullptr;   // e2 closes the transect reduction (K3)
        bool has_mid = false, has_k3 = false;
    };
    std::vector<TimedLaunch> ev;     // pool: created once (nf_field_timing reserves), re-used after every timing_read
    size_t ev_used = 0;              // launches recorded since the last timing_read
    long ev_dropped = 0;             // launches not recorded because the pool was at its cap
    double last_flux_ms = 0.0, last_expand_ms = 0.0, last_k3_ms = 0.0;   // split of the last timing_read
    // hipGraph of one compute_all pass (launch-bound small grids: 4 launches per time step)
    hipGraphExec_t graph_exec = nullptr;
    double *graph_rows = nullptr;
    long graph_version = -1, version = 0;  // version is bumped by every call that changes what a pass launches
};

// what a captured graph of the pass depends on: the field's own settings and every tuning knob
static long field_pass_version(const nf_field *f) { return f->version + tuning_version() + g_knob_version; }

static void field_drop_graph(nf_field *f)
{
    if (f->graph_exec) (void)hipGraphExecDestroy(f->graph_exec);
    f->graph_exec = nullptr;
    f->graph_rows = nullptr;
    f->graph_version = -1;
}

static int field_free_geometry(nf_field *f)
{
    f->geo = {};
    // the locator cache and the lent grid describe the corner table that was just freed: gone with it, on EVERY path out of
    // set_bounds (an early return used to leave boxes keyed on the freed pointer, which hipMalloc often hands out again:
    // round-5 advisor)
    {
        std::lock_guard<std::mutex> lock(f->grid_view.boxes.mtx);
        f->grid_view.boxes.release();
    }
    f->grid_view.d_xy = nullptr;
    f->grid_view.ncell = 0;
    ++f->grid_view.version;
    f->weights_built = false;
    return NF_OK;
}

static int elem_size(int dtype) { return dtype == NF_F32 ? 4 : 8; }

static void field_drop_events(nf_field *f)
{
    for (auto &t : f->ev)
        for (hipEvent_t e : {t.e0, t.mid, t.e1, t.e2})
            if (e) (void)hipEventDestroy(e);
    f->ev.clear();
    f->ev_used = 0;
    f->ev_dropped = 0;
}

// event triples are created outside the timed region (nf_field_timing(n) reserves n) and re-used; the pool never grows
// past kMaxTimedLaunches, so a caller that never reads the timing does not leak events
constexpr size_t kMaxTimedLaunches = 1 << 16;
static int field_reserve_events(nf_field *f, size_t n)
{
    if (n > kMaxTimedLaunches) n = kMaxTimedLaunches;
    while (f->ev.size() < n) {   // an entry joins the pool only when all of its events exist
        nf_field::TimedLaunch t;
        hipError_t err = hipSuccess;
        for (hipEvent_t *e : {&t.e0, &t.mid, &t.e1, &t.e2})
            if (err == hipSuccess) err = hipEventCreate(e);
        if (err != hipSuccess) {
            for (hipEvent_t e : {t.e0, t.mid, t.e1, t.e2})
                if (e) (void)hipEventDestroy(e);
            NF_HIP(err);
        }
        f->ev.push_back(t);
    }
    return NF_OK;
}

// The flux launch of a step: K1, or with per-cell thicknesses (ct) the kernel of nf_cellthick.hip into the signed planes a.iV
// points at, followed -- unless the step is signed-only -- by the expansion into the other four, as in K1's split store form
static int field_flux_kernels(nf_field *f, FluxArgs &a, const CellThick *ct)
{
    if (!ct) return launch_flux(a, f->stream);
    CellThickArgs c;
    c.in = StepInput{a.u, a.v, a.dtype, a.ncell, a.ny, a.nx, a.z0, a.z1, a.thickness, a.arcE, a.arcN, a.fill, a.fill2, a.scale,
                     a.sverdrup};
    c.th = *ct;
    c.planes = a.iV + a.ncell;
    c.maxbits = a.maxbits;
    NF_TRY(launch_cellthick_flux(c, f->stream));
    if (a.signed_only) return NF_OK;
    if (a.mid_event) {
        NF_HIP(hipEventRecord(a.mid_event, f->stream));
        if (a.mid_recorded) *a.mid_recorded = true;
    }
    return launch_expand_planes(a.iV, a.absU, a.ncell, a.ny, a.nx, f->stream);
}

// one flux launch (and, in the default step, the expansion behind it) on the field's stream; with timing on, bracketed by
// events
static int field_launch_flux(nf_field *f, FluxArgs &a, const CellThick *ct = nullptr)
{
    if (!f->timing) return field_flux_kernels(f, a, ct);
    if (f->ev_used >= kMaxTimedLaunches) {   // nobody reads the timing: keep computing, stop recording
        ++f->ev_dropped;
        return field_flux_kernels(f, a, ct);
    }
    NF_TRY(field_reserve_events(f, f->ev_used + 1));   // no-op when nf_field_timing reserved enough
    const size_t k = f->ev_used++;
    bool mid = false;
    a.mid_event = f->ev[k].mid;
    a.mid_recorded = &mid;
    NF_HIP(hipEventRecord(f->ev[k].e0, f->stream));
    const int rc = field_flux_kernels(f, a, ct);
    a.mid_event = nullptr;
    a.mid_recorded = nullptr;
    f->ev[k].has_mid = mid;
    f->ev[k].has_k3 = false;
    NF_TRY(rc);
    NF_HIP(hipEventRecord(f->ev[k].e1, f->stream));
    return NF_OK;
}

// the transect reduction launched right behind a timed flux launch: e1 .. e2 of the same entry
static int field_timed_k3_end(nf_field *f)
{
    if (!f->timing || f->ev_used == 0 || f->ev_dropped) return NF_OK;
    auto &t = f->ev[f->ev_used - 1];
    NF_HIP(hipEventRecord(t.e2, f->stream));
    t.has_k3 = true;
    return NF_OK;
}

// compact mode: bring planes 0, 3 and the |.| planes up to date with planes 1, 2 of the latest step
static int field_ensure_derived(nf_field *f)
{
    if (!f->derived_stale) return NF_OK;
    NF_TRY(launch_expand_planes(f->geo.iV.get(), f->geo.abs.get(), f->ncell, f->ny, f->nx, f->stream));
    f->derived_stale = false;
    return NF_OK;
}

static Transects field_transects(const nf_field *f) { return Transects{&f->ws, f->tr_off_dev.get(), (int)f->polylines.size()}; }
static int field_row_length(const nf_field *f) { return (int)field_transects(f).row_length(); }

// A static host cell thickness that the handle uploaded has the shape of the upload, not of the field: after a set_bounds or
// set_thickness that changed (nz, ny, nx) nothing may read it (the kernels take its pointer without a size).  The shapes are
// compared, not the byte counts: 2 x 100 and 4 x 50 cells are as many bytes.
static int field_cell_thick_current(const nf_field *f, const char *what)
{
    if (!f->e3.p[0] || !f->e3u_static.get()) return NF_OK;
    if (f->e3_static_nz == f->nz && f->e3_static_ny == f->ny && f->e3_static_nx == f->nx) return NF_OK;
    char buf[320];
    snprintf(buf, sizeof buf,
             ": the static cell thickness was uploaded for (nz, ny, nx) = (%ld, %ld, %ld) and the field is now (%ld, %ld, %ld); "
             "call nf_field_set_cell_thickness again with arrays of the new shape, or clear it with NULL",
             f->e3_static_nz, f->e3_static_ny, f->e3_static_nx, f->nz, f->ny, f->nx);
    NF_REQUIRE(false, NF_ERR_STATE, std::string(what) + buf);
    return NF_OK;
}

// The same rule for a static host set of surfaces that the handle uploaded (nf_field_set_depth_surfaces): it has the (ny, nx) of
// the upload.
static int field_surfaces_current(const nf_field *f, const char *what)
{
    if (!f->surf.m || !f->surf.fixed.get()) return NF_OK;
    if (f->surf.fixed_ny == f->ny && f->surf.fixed_nx == f->nx) return NF_OK;
    char buf[320];
    snprintf(buf, sizeof buf,
             ": the static depth surfaces were uploaded for (ny, nx) = (%ld, %ld) and the field is now (%ld, %ld); "
             "call nf_field_set_depth_surfaces again with arrays of the new shape, or clear them with NULL",
             f->surf.fixed_ny, f->surf.fixed_nx, f->ny, f->nx);
    NF_REQUIRE(false, NF_ERR_STATE, std::string(what) + buf);
    return NF_OK;
}

// the state every per-step computation needs; `what` prefixes the message ("compute", "compute_profile", ...)
static int field_ready(const nf_field *f, const char *what, bool weights)
{
    NF_REQUIRE(f->geo.arcE.get() && f->thick.get() && f->uv.p[0] && f->uv.p[1], NF_ERR_STATE,
               std::string(what) + ": set_bounds, set_thickness and set_uv first");
    NF_REQUIRE(!weights || f->weights_built, NF_ERR_STATE, std::string(what) + ": build_weights first");
    NF_TRY(field_surfaces_current(f, what));
    return field_cell_thick_current(f, what);
}

// the end of the slabs [s_begin, s_end) of the nt * nz that this rank owns (set_slab_range; s_end < 0: up to the last one)
static long field_slab_end(const nf_field *f)
{
    const long total = f->uv.nt * f->nz;
    return f->s_end < 0 ? total : std::min(f->s_end, total);
}

// the levels [z0, z1) of step t that this rank owns; z0 == z1 (inside [0, nz]) when it owns none of them
struct Levels {
    int z0 = 0, z1 = 0;
};
static Levels field_levels(const nf_field *f, long t)
{
    const long s_end = field_slab_end(f);
    long lo = t * f->nz, hi = (t + 1) * f->nz;
    if (lo < f->s_begin) lo = std::min(f->s_begin, hi);
    if (hi > s_end) hi = std::max(s_end, lo);
    return {(int)(lo - t * f->nz), (int)(hi - t * f->nz)};
}

// the steps of a pass with an owned slab, [ta, tb), and the whole steps [wa, wb) among them: the ones a pair may take (a
// partial first or last step is reduced on its own).  All zero when the rank owns nothing.
struct PassSteps {
    long ta = 0, tb = 0, wa = 0, wb = 0;
};
static PassSteps field_pass_steps(const nf_field *f)
{
    const long s_end = field_slab_end(f), s_begin = std::min(f->s_begin, s_end);
    PassSteps p;
    if (s_end <= s_begin) return p;
    p.ta = s_begin / f->nz;            // first step with an owned slab
    p.tb = (s_end - 1) / f->nz + 1;    // one past the last
    p.wa = s_begin > p.ta * f->nz ? p.ta + 1 : p.ta;
    p.wb = std::max(p.wa, s_end < p.tb * f->nz ? p.tb - 1 : p.tb);
    return p;
}

// Step t of a (nt, nz, ncell) array of the field dtype as the kernels read it: a device-resident array in place, a
// host-resident one staged into `buf` -- the owned levels only, at their place in one step (PCIe-inclusive path)
static int field_stage(nf_field *f, Series &s, int which, long t, Levels lv, const void **out)
{
    const size_t es = elem_size(f->uv.dtype), step_bytes = (size_t)f->nz * f->ncell * es;
    const char *base = (const char *)s.p[which] + (size_t)t * step_bytes;
    if (s.on_device) {
        *out = base;
        return NF_OK;
    }
    DevArray<char> *buf = &s.stage[which];
    NF_TRY(buf->reserve(step_bytes));
    const size_t off = (size_t)lv.z0 * f->ncell * es, len = (size_t)(lv.z1 - lv.z0) * f->ncell * es;
    NF_HIP(hipMemcpyAsync(buf->get() + off, base + off, len, hipMemcpyHostToDevice, f->stream));
    *out = buf->get();
    return NF_OK;
}

// what the per-step kernels read of step t: uo / vo (staged when host-resident), the grid and the levels lv
static int field_step_input(nf_field *f, long t, Levels lv, StepInput *in)
{
    NF_TRY(field_stage(f, f->uv, 0, t, lv, &in->u));
    NF_TRY(field_stage(f, f->uv, 1, t, lv, &in->v));
    in->dtype = f->uv.dtype;
    in->ncell = f->ncell;
    in->ny = f->ny;
    in->nx = f->nx;
    in->z0 = lv.z0;
    in->z1 = lv.z1;
    in->thickness = f->thick.get();
    in->arcE = f->geo.arcE.get();
    in->arcN = f->geo.arcN.get();
    in->fill = f->uv.fill;
    in->fill2 = f->uv.fill2;
    in->scale = kEarthRadiusSv / 1.e6;   // field.py:226
    in->sverdrup = f->sverdrup;
    return NF_OK;
}

// The "matches uo/vo" rule of a series that is read beside them: their dtype, and their nt (kStaticOk: or one step).  w
// prefixes the message and `noun` names the series.  The setters word some of it in their own way: kNameDtypes, kCountSteps.
enum : int { kStaticOk = 1, kNameDtypes = 2, kCountSteps = 4 };
static int field_matches_uv(const nf_field *f, int dtype, long nt, const std::string &w, const char *noun, int how = 0)
{
    const std::string the = w + ": the " + noun;
    char buf[160];
    if (dtype != f->uv.dtype) {
        if (!(how & kNameDtypes)) NF_REQUIRE(false, NF_ERR_ARG, the + "'s dtype differs from the dtype of uo/vo");
        snprintf(buf, sizeof buf, "'s dtype is %s, uo/vo are %s", dtype == NF_F32 ? "float32" : "float64",
                 f->uv.dtype == NF_F32 ? "float32" : "float64");
        NF_REQUIRE(false, NF_ERR_ARG, the + buf);
    }
    if (nt != f->uv.nt && !((how & kStaticOk) && nt == 1)) {
        if (!(how & kCountSteps)) NF_REQUIRE(false, NF_ERR_ARG, the + "'s nt differs from the nt of uo/vo");
        snprintf(buf, sizeof buf, (how & kStaticOk) ? " has nt = %ld time steps, need 1 (static) or the %ld of uo/vo"
                                                    : " has nt = %ld time steps, uo/vo have %ld", nt, f->uv.nt);
        NF_REQUIRE(false, NF_ERR_ARG, the + buf);
    }
    return NF_OK;
}

// the per-cell thicknesses that go with step t (none set: th->e3u stays nullptr): a static array is its one step, a
// host-resident time-varying one is staged like uo / vo
static int field_cell_thick(nf_field *f, long t, Levels lv, CellThick *th)
{
    *th = CellThick{};
    if (!f->e3.p[0]) return NF_OK;
    NF_TRY(field_matches_uv(f, f->e3.dtype, f->e3.nt, "compute", "cell thickness", kStaticOk));
    const long tt = f->e3.nt == 1 ? 0 : t;
    NF_TRY(field_stage(f, f->e3, 0, tt, lv, &th->e3u));
    NF_TRY(field_stage(f, f->e3, 1, tt, lv, &th->e3v));
    th->fill = f->e3.fill;
    th->fill2 = f->e3.fill2;
    return NF_OK;
}

// the forms that do not take per-cell thicknesses yet: refused while one is set
static int field_no_cell_thick(const nf_field *f, const char *what)
{
    NF_REQUIRE(!f->e3.p[0], NF_ERR_STATE,
               std::string(what) + ": this form does not take per-cell thicknesses yet and a cell thickness is set; "
                                   "nf_field_set_cell_thickness(NULL) clears it");
    return NF_OK;
}

// K1's arguments for a step: FluxArgs begins with the fields of StepInput, in the same order; its outputs are the caller's
static FluxArgs flux_args(const StepInput &in)
{
    return FluxArgs{in.u, in.v, in.dtype, in.ncell, in.ny, in.nx, in.z0, in.z1, in.thickness, in.arcE, in.arcN, in.fill,
                    in.fill2, in.scale, in.sverdrup};
}

// K3 over planes of this field's grid, read through their two signed members, with the field's weights and transects
static int field_integral(nf_field *f, const double *planes, double *scratch, double *rows, int nsteps = 1,
                          long data_stride = 0, long row_stride = 0)
{
    const Transects tr = field_transects(f);
    return launch_integral(f->ws, planes, f->ncell, 2, f->nx, tr.tr_offsets_dev, tr.ntransect, scratch, rows, f->stream, nsteps,
                           data_stride, row_stride);
}

// a synchronous entry point: `step` writes n doubles into `buf`, a device buffer of the field's own, which are copied to `host`
// (nullptr: not copied); the stream is synchronized either way
template <typename Step>
static int field_sync(nf_field *f, DevArray<double> &buf, size_t n, double *host, Step step)
{
    NF_TRY(buf.reserve(n > 0 ? n : 1));
    NF_TRY(step(buf.get()));
    if (host && n > 0) NF_HIP(hipMemcpyAsync(host, buf.get(), sizeof(double) * n, hipMemcpyDeviceToHost, f->stream));
    NF_HIP(hipStreamSynchronize(f->stream));
    return NF_OK;
}

// how field_step_async runs a step of a per-step pass
struct StepForm {
    // a step of the pass that another step follows: its planes are overwritten before anybody but K3 can read them, so
    // only the two signed planes are stored (the f64 flux kernel in its signed-only form, no f32 expansion)
    bool inner = false;
    // the step's signed values go to `pair_buf` (2 * ncell doubles) instead of the resident planes, and no reduction is
    // launched: a step of a pair, reduced by field_pair_async.  The handle's resident state (planes, derived_stale) is not touched.
    double *pair_buf = nullptr;
    // ... as K1's interleaved stream instead of the two planes [eU | eV]
    bool interleaved = false;
};

// one time step on the field's stream; row_dev receives [segments | transects]
static int field_step_async(nf_field *f, long t, double *row_dev, StepForm form = {})
{
    const int rowlen = field_row_length(f);
    const bool reduce = row_dev && rowlen > 0 && !form.pair_buf;
    NF_TRY(field_ready(f, "compute", reduce));
    NF_REQUIRE(t >= 0 && t < f->uv.nt, NF_ERR_ARG, "compute: time index out of range");
    const Levels lv = field_levels(f, t);
    if (lv.z1 <= lv.z0) {  // this rank owns no slab of step t: contributes zeros
        if (row_dev && rowlen > 0) NF_HIP(hipMemsetAsync(row_dev, 0, sizeof(double) * rowlen, f->stream));
        return NF_OK;
    }
    StepInput in;
    NF_TRY(field_step_input(f, t, lv, &in));
    CellThick ct;
    NF_TRY(field_cell_thick(f, t, lv, &ct));
    FluxArgs a = flux_args(in);
    a.iV = f->geo.iV.get();
    // a pair buffer holds planes 1 and 2 only: the signed-only kernel stores to iV + ncell and iV + 2 * ncell, nothing below;
    // the interleaved form stores its one stream at iV
    if (form.pair_buf) a.iV = form.interleaved ? form.pair_buf : form.pair_buf - f->ncell;
    a.absU = f->geo.abs.get();
    a.absV = f->geo.abs.get() + f->ncell;
    a.maxbits = f->geo.maxbits.get();
    // A rank of a sharded run that owns only PART of this step's levels (slab sharding cuts inside a time step) produces
    // partial sums: its south / west copies and |.| planes mean nothing (only a step owned whole has full-field outputs),
    // the transect reduction reads the two signed planes only, so the step runs in the signed-only form and the four derived
    // planes are written on demand (read_step / device_ptr), exactly as in the compact mode.  0.116 ms per such launch at
    // the C4 size; the rows are bit-identical (test_slab_sharding_sums_to_full).  nf_tuning_set("partial_step_planes", 1) keeps the
    // six-plane epilogue on partial steps (the before / after measurement of profiles/r04_rank_emulation.txt).
    const bool partial = (lv.z0 > 0 || lv.z1 < (int)f->nz) && !g_partial_full;
    // (the cell-thickness kernel stores the signed planes in every form, one cell per lane included)
    a.signed_only = (f->compact || partial || form.inner) && (ct.e3u || flux_supports_signed_only(a));
    NF_REQUIRE(!form.pair_buf || a.signed_only, NF_ERR_STATE, "compute: a step into a pair buffer must be signed-only");
    NF_REQUIRE(!form.interleaved || (form.pair_buf && !ct.e3u && !partial && flux_supports_interleaved(a)), NF_ERR_STATE,
               "compute: the interleaved form is a whole step of a pair on K1's two-field kernel");
    a.interleaved = form.interleaved;
    if (!form.pair_buf) f->derived_stale = a.signed_only != 0;
    NF_TRY(field_launch_flux(f, a, ct.e3u ? &ct : nullptr));
    if (reduce) {
        NF_TRY(field_integral(f, f->geo.iV.get(), f->scratch.get(), row_dev));
        NF_TRY(field_timed_k3_end(f));
    }
    return NF_OK;
}

// The opening of the calls that reduce the raw fields of step t into `nrows` rows at rows_dev (`what` prefixes the messages):
// checks the time index and, where a tracer is read (tracer = 1; 2: the class field too), its dtype and nt; *lv: the levels to run the kernels on.  None when a row
// is empty or this rank owns no slab of step t: its rows are then exact zeros, so that the ranks' rows add up to the full ones.
static int field_raw_step_begin(nf_field *f, const char *what, long t, int tracer, double *rows_dev, size_t nrows, Levels *lv)
{
    const std::string w(what);
    NF_REQUIRE(t >= 0 && t < f->uv.nt, NF_ERR_ARG, w + ": time index out of range");
    if (tracer) NF_TRY(field_matches_uv(f, f->tau.dtype, f->tau.nt, w, "tracer"));
    if (tracer == 2 && f->sig.p[0])   // a call that reads the class field
        NF_TRY(field_matches_uv(f, f->sig.dtype, f->sig.nt, w, "class tracer"));
    const size_t rowlen = field_row_length(f);
    *lv = rowlen > 0 ? field_levels(f, t) : Levels{};
    if (rowlen > 0 && lv->z1 <= lv->z0) NF_HIP(hipMemsetAsync(rows_dev, 0, sizeof(double) * rowlen * nrows, f->stream));
    return NF_OK;
}

// Step t of the tracer or the class tracer (staged when host-resident) with its markers.  The reference is the tracer's -- the
// class tracer has none -- and the wrap rule is the tracer's for both.
static int field_tracer_input(nf_field *f, Series &s, long t, Levels lv, TracerIn *in)
{
    NF_TRY(field_stage(f, s, 0, t, lv, &in->tau));
    in->fill = s.fill;
    in->fill2 = s.fill2;
    in->ref = &s == &f->tau ? f->tau_ref : 0.0;
    in->wrap_x = f->tau_wrap;
    return NF_OK;
}

// The tracer inputs of a product that bins by the class field -- the class tracer when one is set, else the tracer -- at step t:
// *cls, the class field on the levels cls_lv, and *carry (nullptr: none), the tracer on the levels lv.  cls_lv is lv, or lv with
// the halo of the remap (field_halo_levels): a host-resident class field is staged with it, an HBM one is read in place.
static int field_class_inputs(nf_field *f, long t, Levels lv, Levels cls_lv, TracerIn *cls, TracerIn *carry)
{
    NF_TRY(field_tracer_input(f, f->tau, t, f->sig.p[0] ? lv : cls_lv, cls));
    if (carry) *carry = *cls;                                                  // the tracer is carried ...
    if (f->sig.p[0]) NF_TRY(field_tracer_input(f, f->sig, t, cls_lv, cls));   // ... and binned by the class tracer
    return NF_OK;
}

// the levels that the remap kernels read the class field on: one above and one below the owned ones
static Levels field_halo_levels(const nf_field *f, Levels lv) { return {std::max(lv.z0 - 1, 0), std::min(lv.z1 + 1, (int)f->nz)}; }

// The window knob and the run sums of a windowed product (class, remap, depth, surface) in the arguments *a: the field's class
// scratch, grown to the window per record.
template <typename Args>
static int field_class_window(nf_field *f, Args *a)
{
    a->window = g_class_window;
    NF_TRY(f->class_scratch.reserve((size_t)f->ws.nrec * a->window));
    a->scratch = f->class_scratch.get();
    a->scratch_len = f->class_scratch.size();
    return NF_OK;
}

// A product that is written whole, `doubles` of it at rows_dev, by a kernel that stores the owned levels alone: zeros for the
// others, in every block, when this rank owns a part of the step (or nothing of it)
static int field_zero_unowned_levels(nf_field *f, Levels lv, double *rows_dev, size_t doubles)
{
    if (lv.z0 > 0 || lv.z1 < f->nz) NF_HIP(hipMemsetAsync(rows_dev, 0, sizeof(double) * doubles, f->stream));
    return NF_OK;
}

// Depth-resolved rows of step t on the field's stream: prof_dev (nz, row_length), row z = the flux carried by level z alone.
// Reads the raw fields and the records; leaves the resident planes, |.| arrays, running max, version and a captured pass
// alone.  Levels this rank does not own get zeros.  The caller has checked field_ready (with the weights).
// tracer = true: every term times the carried tracer at its face (nf_field_compute_tracer_profile), with a scratch of its own.
static int field_profile_async(nf_field *f, long t, double *prof_dev, bool tracer = false)
{
    Levels lv;
    NF_TRY(field_raw_step_begin(f, tracer ? "compute_tracer_profile" : "compute_profile", t, tracer ? 1 : 0, prof_dev,
                                (size_t)f->nz, &lv));
    if (lv.z1 <= lv.z0) return NF_OK;
    const size_t rowlen = field_row_length(f);
    if (lv.z0 > 0) NF_HIP(hipMemsetAsync(prof_dev, 0, sizeof(double) * rowlen * (size_t)lv.z0, f->stream));   // not owned
    if (lv.z1 < f->nz)
        NF_HIP(hipMemsetAsync(prof_dev + (size_t)lv.z1 * rowlen, 0, sizeof(double) * rowlen * (size_t)(f->nz - lv.z1),
                              f->stream));
    DevArray<double> &scratch = tracer ? f->tprof_scratch : f->prof_scratch;
    NF_TRY(scratch.reserve((size_t)f->ws.nrec * (tracer ? tracer_profile_chunk(f->uv.dtype) : kProfileChunk)));
    ProfileArgs a;
    NF_TRY(field_step_input(f, t, lv, &a.in));
    if (tracer) {
        NF_TRY(field_tracer_input(f, f->tau, t, lv, &a.t));
    } else {
        NF_TRY(field_cell_thick(f, t, lv, &a.th));
    }
    a.tr = field_transects(f);
    a.scratch = scratch.get();
    a.scratch_len = scratch.size();
    a.prof = prof_dev;
    return launch_profile(a, f->stream);
}

// Section area and area-weighted tracer of step t on the field's stream: rows_dev (2, nz, row_length) = A, T, written whole.
// Owned levels only, exact zeros elsewhere.  Reads the raw fields, the tracer, the cell thickness when one is set and the
// records; the resident planes, |.| arrays, running max, last row, tracer planes, version and a captured pass stay as they are.
static int field_area_async(nf_field *f, long t, double *rows_dev)
{
    Levels lv;
    NF_TRY(field_raw_step_begin(f, "compute_area_profile", t, 1, rows_dev, 2 * (size_t)f->nz, &lv));
    if (lv.z1 <= lv.z0) return NF_OK;
    NF_TRY(field_zero_unowned_levels(f, lv, rows_dev, (size_t)field_row_length(f) * 2 * (size_t)f->nz));   // in both blocks
    NF_TRY(f->area_scratch.reserve((size_t)f->ws.nrec * 2 * area_chunk_now(f->uv.dtype)));
    AreaArgs a;
    NF_TRY(field_step_input(f, t, lv, &a.in));
    NF_TRY(field_tracer_input(f, f->tau, t, lv, &a.t));
    NF_TRY(field_cell_thick(f, t, lv, &a.th));
    a.tr = field_transects(f);
    a.scratch = f->area_scratch.get();
    a.scratch_len = f->area_scratch.size();
    a.rows = rows_dev;
    a.nz = f->nz;
    return launch_area_profile(a, f->stream);
}

// Gross transports of step t on the field's stream: rows_dev (2, nz, row_length) = P, N, written whole.  carry: the terms of the
// tracer profile instead of those of the volume profile, split by the direction of the water all the same.  Owned levels only,
// exact zeros elsewhere.  Reads the raw fields, the tracer (carry), the cell thickness when one is set and the records; the
// resident planes, |.| arrays, running max, last row, tracer planes, version and a captured pass stay as they are.
static int field_gross_async(nf_field *f, long t, bool carry, double *rows_dev)
{
    Levels lv;
    NF_TRY(field_raw_step_begin(f, "compute_gross_profile", t, carry ? 1 : 0, rows_dev, 2 * (size_t)f->nz, &lv));
    if (lv.z1 <= lv.z0) return NF_OK;
    NF_TRY(field_zero_unowned_levels(f, lv, rows_dev, (size_t)field_row_length(f) * 2 * (size_t)f->nz));   // in both blocks
    NF_TRY(f->gross_scratch.reserve((size_t)f->ws.nrec * 2 * gross_chunk_now(f->uv.dtype, carry, f->e3.p[0] != nullptr)));
    GrossArgs a;
    NF_TRY(field_step_input(f, t, lv, &a.in));
    if (carry) NF_TRY(field_tracer_input(f, f->tau, t, lv, &a.t));
    NF_TRY(field_cell_thick(f, t, lv, &a.th));
    a.tr = field_transects(f);
    a.scratch = f->gross_scratch.get();
    a.scratch_len = f->gross_scratch.size();
    a.rows = rows_dev;
    a.nz = f->nz;
    return launch_gross_profile(a, f->stream);
}

// Crossings of step t on the field's stream: out_dev (carry ? 4 : 2, nz, ws.nrec), written whole: the planes q, g (volume
// form) or q, c, a, b (carried form) per record and level, no reduction.  Owned levels only, exact zeros elsewhere.  Reads the
// raw fields, the tracer (carry), the cell thickness when one is set and the records; the resident planes, |.| arrays, running
// max, last row, tracer planes, class / joint rows, version and a captured pass stay as they are.
static int field_crossings_async(nf_field *f, long t, bool carry, double *out_dev)
{
    NF_REQUIRE(t >= 0 && t < f->uv.nt, NF_ERR_ARG, "compute_crossings: time index out of range");
    if (carry) NF_TRY(field_matches_uv(f, f->tau.dtype, f->tau.nt, "compute_crossings", "tracer"));
    const size_t nrec = (size_t)f->ws.nrec, nplanes = carry ? 4 : 2;
    if (nrec == 0) return NF_OK;
    const Levels lv = field_levels(f, t);
    NF_TRY(field_zero_unowned_levels(f, lv, out_dev, nplanes * (size_t)f->nz * nrec));   // in every plane
    if (lv.z1 <= lv.z0) return NF_OK;
    CrossingArgs a;
    NF_TRY(field_step_input(f, t, lv, &a.in));
    if (carry) NF_TRY(field_tracer_input(f, f->tau, t, lv, &a.t));
    NF_TRY(field_cell_thick(f, t, lv, &a.th));
    a.ws = &f->ws;
    a.out = out_dev;
    a.nz = f->nz;
    return launch_crossing_terms(a, f->stream);
}

// Tracer transport of step t on the field's stream: K1tau into geo.tr_planes, then K3 over them into row_dev
// [segments | transects].  Owned levels only (partial sums), zeros for a step this rank does not touch.  Reads the raw fields
// and the records; the resident planes, |.| arrays, running max, version and a captured pass stay as they are.
static int field_tracer_step_async(nf_field *f, long t, double *row_dev)
{
    NF_TRY(field_ready(f, "compute_tracer", true));
    Levels lv;
    NF_TRY(field_raw_step_begin(f, "compute_tracer", t, 1, row_dev, 1, &lv));
    if (lv.z1 <= lv.z0) return NF_OK;
    TracerArgs a;
    NF_TRY(field_step_input(f, t, lv, &a.in));
    NF_TRY(field_tracer_input(f, f->tau, t, lv, &a.t));
    NF_TRY(field_cell_thick(f, t, lv, &a.th));
    NF_TRY(f->geo.tr_planes.reserve((size_t)f->ncell * 2));
    a.planes = f->geo.tr_planes.get();
    NF_TRY(launch_tracer_flux(a, f->stream));
    // K3 reads the two signed members of [4][ncell] planes at +ncell and +2 ncell: the tracer planes sit at +ncell
    return field_integral(f, f->geo.tr_planes.get() - f->ncell, f->scratch.get(), row_dev);
}

// the calls of the class transport need a tracer and class edges: checked before a device is needed
static int field_class_ready(const nf_field *f, const char *what, bool /*carry*/ = false)
{
    NF_REQUIRE(f->tau.p[0], NF_ERR_STATE, std::string(what) + ": set_tracer first");
    NF_REQUIRE(!f->class_edges.host.empty(), NF_ERR_STATE, std::string(what) + ": set_class_edges first");
    return field_ready(f, what, true);
}

// Volume transport in tracer classes of step t on the field's stream: rows_dev (nedges + 2, row_length), written whole.
// Owned levels only, exact zeros for a step this rank does not touch.  Reads the raw fields, the tracer and the records; the
// resident planes, |.| arrays, running max, last row, tracer planes, version and a captured pass stay as they are.
// The class field is the class tracer when one is set, else the tracer.  carry = true: the transport of the tracer instead
// of the volume (nf_field_compute_class_tracer_transport).  remap = true: by conservative remapping
// (nf_field_compute_class_remap, launch_class_remap); its kernel reads the class field one level above and one below the owned
// ones, so a host-resident class field is staged with that halo level on each side (an HBM one is read in place).
static int field_class_step_async(nf_field *f, long t, double *rows_dev, bool carry = false, bool remap = false)
{
    const int nedges = (int)f->class_edges.host.size();
    const char *what = remap ? "compute_class_remap" : carry ? "compute_class_tracer_transport" : "compute_class_transport";
    Levels lv;
    NF_TRY(field_raw_step_begin(f, what, t, 2, rows_dev, (size_t)nedges + 2, &lv));
    if (lv.z1 <= lv.z0) return NF_OK;
    NF_TRY(f->class_edges.upload((size_t)kMaxClassEdges, f->stream));
    ClassArgs a;
    NF_TRY(field_class_window(f, &a));
    NF_TRY(field_step_input(f, t, lv, &a.in));
    NF_TRY(field_class_inputs(f, t, lv, remap ? field_halo_levels(f, lv) : lv, &a.cls, carry ? &a.carry : nullptr));
    a.edges = f->class_edges.dev.get();
    a.nedges = nedges;
    a.tr = field_transects(f);
    a.rows = rows_dev;
    a.remap_nz = (int)f->nz;   // read by launch_class_remap only
    return remap ? launch_class_remap(a, f->stream) : launch_class_transport(a, f->stream);
}

// Transports in depth bins of step t on the field's stream (nf_field_compute_depth_transport): rows_dev (nedges + 2,
// row_length), written whole.  Terms of the owned levels only, exact zeros for a step this rank does not touch; the interface
// depths are summed from level 0, so a cell thickness is read -- and a host-resident time-varying one staged -- for the levels
// [0, z1) of the step.  Reads the raw fields, the tracer (carry), the thickness and the records; the resident planes, |.|
// arrays, running max, last row, tracer planes, class / joint rows, version and a captured pass stay as they are.
static int field_depth_step_async(nf_field *f, long t, bool carry, double *rows_dev)
{
    const int nedges = (int)f->depth_edges.host.size();
    Levels lv;
    NF_TRY(field_raw_step_begin(f, "compute_depth_transport", t, carry ? 1 : 0, rows_dev, (size_t)nedges + 2, &lv));
    if (lv.z1 <= lv.z0) return NF_OK;
    NF_TRY(f->depth_edges.upload((size_t)kMaxClassEdges, f->stream));
    DepthArgs a;
    NF_TRY(field_class_window(f, &a));
    NF_TRY(field_step_input(f, t, lv, &a.in));
    if (carry) NF_TRY(field_tracer_input(f, f->tau, t, lv, &a.t));
    NF_TRY(field_cell_thick(f, t, Levels{0, lv.z1}, &a.th));
    a.edges = f->depth_edges.dev.get();
    a.nedges = nedges;
    a.top = f->depth_top;
    a.tr = field_transects(f);
    a.rows = rows_dev;
    return launch_depth_transport(a, f->stream);
}

// Transports between the surfaces of step t on the field's stream (nf_field_compute_surface_transport): rows_dev (m + 2,
// row_length), written whole.  field_depth_step_async with the surfaces in place of the edges: step t' = t of every surface, or
// 0 of a static set; a host-resident time-varying set is staged, the m planes of the step, into a buffer of the handle.
static int field_surface_step_async(nf_field *f, long t, bool carry, double *rows_dev)
{
    nf_field::Surfaces &sf = f->surf;
    Levels lv;
    NF_TRY(field_raw_step_begin(f, "compute_surface_transport", t, carry ? 1 : 0, rows_dev, (size_t)sf.m + 2, &lv));
    if (lv.z1 <= lv.z0) return NF_OK;
    NF_TRY(field_matches_uv(f, sf.dtype, sf.nt, "compute_surface_transport", "depth surfaces", kStaticOk));
    SurfaceArgs a;
    NF_TRY(field_class_window(f, &a));
    NF_TRY(field_step_input(f, t, lv, &a.in));
    if (carry) NF_TRY(field_tracer_input(f, f->tau, t, lv, &a.t));
    NF_TRY(field_cell_thick(f, t, Levels{0, lv.z1}, &a.th));
    const size_t plane = (size_t)f->ncell * elem_size(f->uv.dtype);
    const size_t off = (sf.nt == 1 ? 0 : (size_t)t) * plane;
    if (!sf.on_device) NF_TRY(sf.stage.reserve(plane * sf.m));
    for (int q = 0; q < sf.m; ++q) {
        const char *src = (const char *)sf.p[q] + off;
        if (!sf.on_device) {
            char *dst = sf.stage.get() + (size_t)q * plane;
            NF_HIP(hipMemcpyAsync(dst, src, plane, hipMemcpyHostToDevice, f->stream));
            src = dst;
        }
        a.sf.p[q] = src;
    }
    a.sf.m = sf.m;
    a.sf.fill = sf.fill;
    a.sf.fill2 = sf.fill2;
    a.sf.wrap_x = sf.wrap;
    a.top = sf.top;
    a.tr = field_transects(f);
    a.rows = rows_dev;
    return launch_surface_transport(a, f->stream);
}

// the calls of the joint class transport need both tracers and the joint edges: checked before a device is needed
static int field_joint_ready(const nf_field *f, const char *what, bool /*carry*/ = false)
{
    NF_REQUIRE(f->tau.p[0], NF_ERR_STATE, std::string(what) + ": set_tracer first");
    NF_REQUIRE(f->sig.p[0], NF_ERR_STATE, std::string(what) + ": set_class_tracer first");
    NF_REQUIRE(!f->joint_edges.host.empty(), NF_ERR_STATE, std::string(what) + ": set_joint_class_edges first");
    NF_TRY(field_ready(f, what, true));
    return field_no_cell_thick(f, what);
}

static size_t field_joint_rows(const nf_field *f) { return (size_t)(f->joint_na + 2) * (size_t)(f->joint_nb + 2); }

// The term table, flags and run sums of a product that bins a term table (joint classes, gross classes, class area) into
// `nrows` rows, with the window and skip knobs, in the arguments *a: the field's joint buffers, grown to the need of entry_bytes
// per (record, owned level).  11.6 GB on the bench workload: a failure names the size, and nothing falls back to another path.
template <typename Args>
static int field_joint_buffers(nf_field *f, const char *what, size_t entry_bytes, const Levels &lv, size_t nrows, Args *a)
{
    const int window = g_joint_window;
    const size_t nrec = (size_t)f->ws.nrec, blocks = (nrec + kBlock - 1) / kBlock;
    const size_t table_bytes = entry_bytes * nrec * (size_t)(lv.z1 - lv.z0);
    if (f->joint_table.size() == 0 || f->joint_table.size() < table_bytes) {
        if (f->joint_table.alloc(table_bytes) != NF_OK) {
            char buf[256];
            snprintf(buf, sizeof buf, "%s: cannot allocate the term table of %zu bytes (%zu bytes x %zu records x %d owned levels)",
                     what, table_bytes, entry_bytes, nrec, lv.z1 - lv.z0);
            NF_REQUIRE(false, NF_ERR_HIP, buf);
        }
    }
    NF_TRY(f->joint_flags.reserve(blocks * (size_t)joint_flag_words((int)nrows, window)));
    NF_TRY(f->joint_scratch.reserve(nrec * (size_t)window));
    a->window = window;
    a->skip = g_joint_skip;
    a->table = f->joint_table.get();
    a->table_len = f->joint_table.size();
    a->flags = f->joint_flags.get();
    a->flags_len = f->joint_flags.size();
    a->scratch = f->joint_scratch.get();
    a->scratch_len = f->joint_scratch.size();
    return NF_OK;
}

// Transport of step t in joint classes of the tracer (axis A) and the class tracer (axis B) on the field's stream: rows_dev
// ((na + 2) * (nb + 2), row_length), written whole.  Owned levels only, exact zeros for a step this rank does not touch.
// Reads the raw fields, both tracers and the records; the resident planes, |.| arrays, running max, last row, tracer planes,
// 1-D class rows, version and a captured pass stay as they are.  carry: the transport of the tracer instead of the volume.
static int field_joint_step_async(nf_field *f, long t, bool carry, double *rows_dev)
{
    const size_t nrows = field_joint_rows(f);
    Levels lv;
    NF_TRY(field_raw_step_begin(f, "compute_joint_class_transport", t, 2, rows_dev, nrows, &lv));
    if (lv.z1 <= lv.z0) return NF_OK;
    NF_TRY(f->joint_edges.upload(2 * (size_t)kMaxClassEdges, f->stream));
    JointArgs a;
    NF_TRY(field_joint_buffers(f, "compute_joint_class_transport", kJointEntryBytes, lv, nrows, &a));
    NF_TRY(field_step_input(f, t, lv, &a.in));
    NF_TRY(field_tracer_input(f, f->tau, t, lv, &a.ta));
    NF_TRY(field_tracer_input(f, f->sig, t, lv, &a.tb));
    a.carry = carry ? 1 : 0;
    a.edges = f->joint_edges.dev.get();
    a.na = f->joint_na;
    a.nb = f->joint_nb;
    a.tr = field_transects(f);
    a.rows = rows_dev;
    return launch_joint_class_transport(a, f->stream);
}

// Gross (inflow / outflow) transports of step t in the classes of the class field on the field's stream: rows_dev
// (2, nedges + 2, row_length) = P, N, written whole.  Owned levels only, exact zeros for a step this rank does not touch.  The
// class field is the class tracer when one is set, else the tracer; carry: the terms of the class tracer transport instead of
// the volume's, split by the direction of the water all the same.  Unlike the net class forms it takes a cell thickness.  The
// term table, flags and run sums are the joint class transport's buffers, grown to the larger need.  Reads the raw fields, the
// tracers, the cell thickness when one is set and the records; the resident planes, |.| arrays, running max, last row, tracer
// planes, class and joint rows, version and a captured pass stay as they are.
static int field_gross_class_async(nf_field *f, long t, bool carry, double *rows_dev)
{
    const int nedges = (int)f->class_edges.host.size();
    const size_t nrows = 2 * ((size_t)nedges + 2);
    Levels lv;
    NF_TRY(field_raw_step_begin(f, "compute_gross_class_transport", t, 2, rows_dev, nrows, &lv));
    if (lv.z1 <= lv.z0) return NF_OK;
    NF_TRY(f->class_edges.upload((size_t)kMaxClassEdges, f->stream));
    GrossClassArgs a;
    NF_TRY(field_joint_buffers(f, "compute_gross_class_transport", kJointEntryBytes, lv, nrows, &a));
    NF_TRY(field_step_input(f, t, lv, &a.in));
    NF_TRY(field_class_inputs(f, t, lv, lv, &a.cls, carry ? &a.carry : nullptr));
    NF_TRY(field_cell_thick(f, t, lv, &a.th));
    a.edges = f->class_edges.dev.get();
    a.nedges = nedges;
    a.tr = field_transects(f);
    a.rows = rows_dev;
    return launch_gross_class_transport(a, f->stream);
}

// Remapped gross class transports of step t on the field's stream (nf_field_compute_gross_class_remap): rows_dev
// (2, nedges + 2, row_length) = P, N, written whole.  field_class_step_async with remap = true -- the class forms' edges, window
// and scratch, the class field staged with one halo level on each side of the owned range when it is host-resident -- with the
// parts of field_gross_class_async and, unlike the net remap, a cell thickness (owned levels only).  Exact zeros for a step
// this rank does not touch.  Reads the raw fields, the tracers, the cell thickness when one is set and the records; the
// resident planes, |.| arrays, running max, last row, tracer planes, class / joint / depth / surface state, version and a
// captured pass stay as they are.
static int field_gross_remap_async(nf_field *f, long t, bool carry, double *rows_dev)
{
    const int nedges = (int)f->class_edges.host.size();
    Levels lv;
    NF_TRY(field_raw_step_begin(f, "compute_gross_class_remap", t, 2, rows_dev, 2 * ((size_t)nedges + 2), &lv));
    if (lv.z1 <= lv.z0) return NF_OK;
    NF_TRY(f->class_edges.upload((size_t)kMaxClassEdges, f->stream));
    GrossRemapArgs a;
    NF_TRY(field_class_window(f, &a));
    NF_TRY(field_step_input(f, t, lv, &a.in));
    NF_TRY(field_class_inputs(f, t, lv, field_halo_levels(f, lv), &a.cls, carry ? &a.carry : nullptr));
    NF_TRY(field_cell_thick(f, t, lv, &a.th));
    a.edges = f->class_edges.dev.get();
    a.nedges = nedges;
    a.tr = field_transects(f);
    a.rows = rows_dev;
    a.nz = (int)f->nz;
    return launch_gross_class_remap(a, f->stream);
}

// Section area (A) and area-weighted tracer (B) of step t in the classes of the class field on the field's stream: rows_dev
// (2, nedges + 2, row_length) = A, B, written whole.  Owned levels only, exact zeros for a step this rank does not touch.  The
// class field is the class tracer when one is set, else the tracer, which is the carried one either way.  It takes a cell
// thickness, as the area profile does.  The term table, flags and run sums are the joint class transport's buffers, grown to the
// larger need: the table takes two entries per (record, owned level) here.  Reads the raw fields, the tracers, the cell
// thickness when one is set and the records; the resident planes, |.| arrays, running max, last row, tracer planes, class and
// joint rows, version and a captured pass stay as they are.
static int field_class_area_async(nf_field *f, long t, double *rows_dev)
{
    const int nedges = (int)f->class_edges.host.size();
    const size_t nrows = 2 * ((size_t)nedges + 2);
    Levels lv;
    NF_TRY(field_raw_step_begin(f, "compute_class_area", t, 2, rows_dev, nrows, &lv));
    if (lv.z1 <= lv.z0) return NF_OK;
    NF_TRY(f->class_edges.upload((size_t)kMaxClassEdges, f->stream));
    ClassAreaArgs a;
    NF_TRY(field_joint_buffers(f, "compute_class_area", kClassAreaEntryBytes, lv, nrows, &a));
    NF_TRY(field_step_input(f, t, lv, &a.in));
    NF_TRY(field_class_inputs(f, t, lv, lv, &a.cls, &a.carry));   // the tracer is the carried one either way
    NF_TRY(field_cell_thick(f, t, lv, &a.th));
    a.edges = f->class_edges.dev.get();
    a.nedges = nedges;
    a.tr = field_transects(f);
    a.rows = rows_dev;
    return launch_class_area(a, f->stream);
}

// ---- the per-step products: what differs between them, stated once, and the one path of their entry points -------------------
// A per-step product is a result of one time step computed from the raw fields and the records, with two entry points: the
// synchronous one (rows to the host) and `_async` (rows in HBM, on the field's stream).  `what` is the symbol called.
struct Product {
    int (*ready)(const nf_field *f, const char *what, bool carry);    // the checks of the state: before a device is asked for
    size_t (*doubles)(const nf_field *f, bool carry);                 // the size of the result
    int (*step)(nf_field *f, long t, bool carry, double *rows_dev);   // step t on the field's stream
    DevArray<double> nf_field::*buffer = &nf_field::row;              // the buffer of the handle that the synchronous form stages through
    bool empty_runs = false;   // the synchronous form runs the step of an empty result too (the crossings: kept as it was)
};

static int field_product(nf_field **self, const Product &p, const char *what, long t, int carry, double *rows, bool sync)
{
    NF_REQUIRE(self && *self && rows, NF_ERR_ARG, std::string(what) + ": null argument");
    NF_REQUIRE(carry == 0 || carry == 1, NF_ERR_ARG, std::string(what) + ": carry must be 0 or 1");
    nf_field *f = *self;
    NF_TRY(p.ready(f, what, carry != 0));
    NF_NEED_DEVICE();
    if (!sync) return p.step(f, t, carry != 0, rows);
    const size_t n = p.doubles(f, carry != 0);
    if (n == 0 && !p.empty_runs) return NF_OK;
    return field_sync(f, f->*p.buffer, n, rows, [&](double *dev) { return p.step(f, t, carry != 0, dev); });
}

// the carried form of a product needs a tracer
static int field_carry_ready(const nf_field *f, const char *what, bool carry)
{
    NF_REQUIRE(!carry || f->tau.p[0], NF_ERR_STATE, std::string(what) + ": set_tracer first");
    return NF_OK;
}

// The area profile, the gross profile and the crossings ask for a device BEFORE they look at the grid, and name themselves
// without the nf_field_ prefix there: without a GPU a handle that is not ready answers NF_ERR_NO_DEVICE, not NF_ERR_STATE.
// Nobody chose that; it is kept as it was ("adding a product").
static int field_ready_on_device(const nf_field *f, const char *short_name)
{
    NF_NEED_DEVICE();
    return field_ready(f, short_name, true);
}

// the net class forms (step rule, carried, remap) take no cell thickness
static int field_net_class_ready(const nf_field *f, const char *what, bool)
{
    NF_TRY(field_class_ready(f, what));
    return field_no_cell_thick(f, what);
}

static size_t field_rows(const nf_field *f, size_t nrows) { return nrows * (size_t)field_row_length(f); }
static size_t field_class_rows(const nf_field *f, bool) { return field_rows(f, f->class_edges.host.size() + 2); }
static size_t field_two_class_rows(const nf_field *f, bool) { return 2 * field_class_rows(f, false); }

// (the two profiles name themselves without the prefix in the message of field_ready: kept as it was)
static const Product kProfile = {
    [](const nf_field *f, const char *, bool) { return field_ready(f, "compute_profile", true); },
    [](const nf_field *f, bool) { return field_rows(f, (size_t)f->nz); },
    [](nf_field *f, long t, bool, double *rows) { return field_profile_async(f, t, rows); }};
static const Product kTracerProfile = {
    [](const nf_field *f, const char *what, bool) {
        NF_TRY(field_carry_ready(f, what, true));
        NF_TRY(field_no_cell_thick(f, what));
        return field_ready(f, "compute_tracer_profile", true);
    },
    kProfile.doubles,
    [](nf_field *f, long t, bool, double *rows) { return field_profile_async(f, t, rows, true); }};
static const Product kAreaProfile = {
    [](const nf_field *f, const char *what, bool) {
        NF_TRY(field_carry_ready(f, what, true));
        return field_ready_on_device(f, "compute_area_profile");
    },
    [](const nf_field *f, bool) { return field_rows(f, 2 * (size_t)f->nz); },
    [](nf_field *f, long t, bool, double *rows) { return field_area_async(f, t, rows); }};
static const Product kGrossProfile = {
    [](const nf_field *f, const char *what, bool carry) {
        NF_TRY(field_carry_ready(f, what, carry));
        return field_ready_on_device(f, "compute_gross_profile");
    },
    kAreaProfile.doubles,
    [](nf_field *f, long t, bool carry, double *rows) { return field_gross_async(f, t, carry, rows); }};
static const Product kCrossings = {
    [](const nf_field *f, const char *what, bool carry) {
        NF_TRY(field_carry_ready(f, what, carry));
        return field_ready_on_device(f, "compute_crossings");
    },
    [](const nf_field *f, bool carry) { return (carry ? 4 : 2) * (size_t)f->nz * (size_t)f->ws.nrec; },
    [](nf_field *f, long t, bool carry, double *out) { return field_crossings_async(f, t, carry, out); },
    &nf_field::crossings, true};
static const Product kClassTransport = {
    field_net_class_ready, field_class_rows,
    [](nf_field *f, long t, bool, double *rows) { return field_class_step_async(f, t, rows); }};
static const Product kClassTracerTransport = {
    field_net_class_ready, field_class_rows,
    [](nf_field *f, long t, bool, double *rows) { return field_class_step_async(f, t, rows, true); }};
static const Product kClassRemap = {
    field_net_class_ready, field_class_rows,
    [](nf_field *f, long t, bool carry, double *rows) { return field_class_step_async(f, t, rows, carry, true); }};
static const Product kDepthTransport = {
    [](const nf_field *f, const char *what, bool carry) {
        NF_REQUIRE(!f->depth_edges.host.empty(), NF_ERR_STATE, std::string(what) + ": set_depth_edges first");
        NF_TRY(field_carry_ready(f, what, carry));
        return field_ready(f, what, true);
    },
    [](const nf_field *f, bool) { return field_rows(f, f->depth_edges.host.size() + 2); }, field_depth_step_async};
static const Product kSurfaceTransport = {
    [](const nf_field *f, const char *what, bool carry) {
        NF_REQUIRE(f->surf.m > 0, NF_ERR_STATE, std::string(what) + ": set_depth_surfaces first");
        NF_TRY(field_carry_ready(f, what, carry));
        return field_ready(f, what, true);
    },
    [](const nf_field *f, bool) { return field_rows(f, (size_t)f->surf.m + 2); }, field_surface_step_async};
static const Product kJointClassTransport = {
    field_joint_ready, [](const nf_field *f, bool) { return field_rows(f, field_joint_rows(f)); }, field_joint_step_async};
static const Product kGrossClassTransport = {field_class_ready, field_two_class_rows, field_gross_class_async};
static const Product kGrossClassRemap = {field_class_ready, field_two_class_rows, field_gross_remap_async};
static const Product kClassArea = {
    field_class_ready, field_two_class_rows,
    [](nf_field *f, long t, bool, double *rows) { return field_class_area_async(f, t, rows); }};

// steps t and t+1, both owned whole: flux t into geo.pair[0], flux t+1 into the resident planes (which therefore hold the later
// step, as after two single steps), then ONE reduction of both; rows t and t+1 are contiguous in rows_dev.  last: t+1 is the
// last owned step of the pass, which stores what it stores on its own.  interleaved (field_pass_interleaved): the first step
// is stored as K1's interleaved stream, and so is -- into geo.pair[1] -- the second step of a pair that another pair
// follows (last_pair = false): the pass's last pair overwrites the resident planes behind it, so nobody can miss them.
static int field_pair_async(nf_field *f, long t, double *rows_dev, bool last, bool last_pair, bool interleaved)
{
    const int rowlen = field_row_length(f);
    StepForm first, second;
    first.inner = true;
    first.pair_buf = f->geo.pair[0].get();
    first.interleaved = interleaved;
    second.inner = g_inner_signed && !last;
    if (interleaved && second.inner && !last_pair) {
        second.pair_buf = f->geo.pair[1].get();
        second.interleaved = true;
    }
    NF_TRY(field_step_async(f, t, nullptr, first));
    NF_TRY(field_step_async(f, t + 1, nullptr, second));
    const double *uvB = second.pair_buf ? second.pair_buf : f->geo.iV.get() + f->ncell;
    NF_TRY(launch_integral_pair(field_transects(f), first.pair_buf, uvB, f->ncell, f->nx, f->scratch.get(),
                                rows_dev + (size_t)t * rowlen, rowlen, f->stream, first.interleaved, second.interleaved));
    NF_TRY(field_timed_k3_end(f));   // the pair's reduction is timed with the second step's launch
    return NF_OK;
}

// All nt steps in FOUR launches (flux kernel with blockIdx.y = step, then the three reduction kernels): small grids
// are launch-bound (4 launches of a few microseconds per step otherwise).  Needs HBM-resident fields and per-step
// planes (nt x 48 B per cell), so it is used while nt*ncell stays under 32 Mi cell-steps ("batch_cellsteps_m").
static long batch_cell_steps() { return g_batch_cellsteps; }

static bool field_can_batch(const nf_field *f)
{
    // launch-bound grids only: from about a million cells on, one launch per step (with the one-field form of the flux
    // kernel for its few wavefronts) is as fast or faster -- 1440 x 1021: 700 vs 733 us per 4-step pass at float32, 1166 vs
    // 1144 at float64; 2160 x 1080: 1035 vs 1187 and 1863 vs 1928 (tools/size_sweep.py, profiles/r04_size_sweep.txt)
    // (the all-steps-in-one-launch form exists for K1 only: off while a cell thickness is set)
    return g_batch_steps && !f->e3.p[0] && f->uv.on_device && f->uv.nt >= 2 && f->uv.nt < 65536 &&
           f->uv.nt * f->ncell <= batch_cell_steps() && f->ncell <= (1l << 20) && f->weights_built;
}

// the per-step pass reduces its whole steps in pairs: needs the record form of K3 (the unique-edge entries have no pair
// kernel), the second signed planes (field_prepare_pass) and the signed-only flux kernel for the first step of a pair
static bool field_pass_pairs(const nf_field *f)
{
    if (!g_k3_pairs || integral_uses_edges() || !f->geo.pair[0].get() || !f->weights_built) return false;
    // every step starts 16-byte aligned when the first one does: resident fields with a step size that is a multiple of
    // 16 bytes, or steps staged into the (allocation-aligned) staging buffers
    const size_t step_bytes = (size_t)f->nz * f->ncell * elem_size(f->uv.dtype);
    FluxArgs a{};
    a.u = f->uv.on_device ? f->uv.p[0] : nullptr;
    a.v = f->uv.on_device ? f->uv.p[1] : nullptr;
    a.dtype = f->uv.dtype;
    a.ncell = f->ncell;
    return flux_supports_signed_only(a) && (!f->uv.on_device || step_bytes % 16 == 0);
}

// ... and stores the steps of its pairs that nobody else reads interleaved ("pass_inner_interleaved"): K1's own kernel in its
// two-field form only -- not the cell-thickness kernel, not the compact mode, not a launch small enough for the one-field form
static bool field_pass_interleaved(const nf_field *f)
{
    const bool on = g_inner_interleaved < 0 ? f->uv.dtype == NF_F64 : g_inner_interleaved != 0;
    if (!on || f->compact || f->e3.p[0]) return false;
    FluxArgs a{};
    a.u = f->uv.on_device ? f->uv.p[0] : nullptr;
    a.v = f->uv.on_device ? f->uv.p[1] : nullptr;
    a.dtype = f->uv.dtype;
    a.ncell = f->ncell;
    return flux_supports_interleaved(a);
}

// device memory a per-step pass may need, allocated before the pass is launched or captured: the buffers of the steps of a
// pair that do not go to the resident planes.  Nothing is allocated for a pass that takes no pairs (knob off, fewer than two
// whole steps owned, the edge-entry form of K3), and the second buffer only for a pass of two pairs or more that interleaves.
static int field_prepare_pass(nf_field *f)
{
    if (!g_k3_pairs || integral_uses_edges() || !f->geo.iV.get()) return NF_OK;
    const PassSteps p = field_pass_steps(f);
    if (p.wb - p.wa < 2) return NF_OK;
    if (!f->geo.pair[0].get()) NF_TRY(f->geo.pair[0].alloc((size_t)f->ncell * 2));
    if (!f->geo.pair[1].get() && p.wb - p.wa >= 4 && field_pass_interleaved(f)) NF_TRY(f->geo.pair[1].alloc((size_t)f->ncell * 2));
    return NF_OK;
}

// every time step of a pass, one after the other.  A rank of a multi-GPU run owns a contiguous range of steps (slab
// sharding): the rows of all the others are zeroed with two memsets instead of one per step (at 8 ranks that is 84 tiny
// launches per pass saved), and only the owned steps are walked.
// the rows of the steps before and after this rank's own: exact zeros
static int field_zero_unowned_rows(nf_field *f, double *rows_dev)
{
    const int rowlen = field_row_length(f);
    const PassSteps p = field_pass_steps(f);
    if (rowlen <= 0) return NF_OK;
    if (p.ta > 0) NF_HIP(hipMemsetAsync(rows_dev, 0, sizeof(double) * rowlen * (size_t)p.ta, f->stream));
    if (p.tb < f->uv.nt)
        NF_HIP(hipMemsetAsync(rows_dev + (size_t)p.tb * rowlen, 0, sizeof(double) * rowlen * (size_t)(f->uv.nt - p.tb),
                              f->stream));
    return NF_OK;
}

// zero_rows = false: the caller zeroes the other ranks' rows itself -- a captured pass, whose memsets stay out of the graph.
// Observed once (tests/test_gpu_reuse_products.py, seed 14): with the memsets as nodes of the graph, a replay that followed a
// flux call and other allocations of the process left other bytes than zeros in the row of a step that is not owned.  Nothing
// else in the library writes such a row, but the cause is not established -- whether the replayed memset node or something
// else -- so this is a workaround: the memsets are issued on the stream before every launch of the graph.  Their cost (at
// most two small stream memsets per pass of a sharded rank, none for a rank that owns every step) was not measured on its own.
static int field_all_steps_direct(nf_field *f, double *rows_dev, bool zero_rows = true)
{
    const int rowlen = field_row_length(f);
    const PassSteps p = field_pass_steps(f);
    if (zero_rows) NF_TRY(field_zero_unowned_rows(f, rows_dev));
    const bool pairs = field_pass_pairs(f) && rowlen > 0;
    // an odd number of whole steps leaves one of them single: the first, so that the last pair ends on the last whole step
    // and every pair's second step lands in the resident planes
    const long pa = pairs ? p.wa + (p.wb - p.wa) % 2 : p.wb;
    // (a pass of two pairs or more interleaves only with the second buffer that field_prepare_pass gave it)
    const bool interleaved = pairs && field_pass_interleaved(f) && (p.wb - pa < 4 || f->geo.pair[1].get());
    for (long t = p.ta; t < p.tb;) {
        const bool last = t + 1 == p.tb;
        if (t >= pa && t + 1 < p.wb) {
            NF_TRY(field_pair_async(f, t, rows_dev, t + 2 == p.tb, t + 2 == p.wb, interleaved));
            t += 2;
        } else {
            StepForm form;
            form.inner = g_inner_signed && !last;
            NF_TRY(field_step_async(f, t, rows_dev + (size_t)t * rowlen, form));
            t += 1;
        }
    }
    return NF_OK;
}

static int field_all_steps_batched(nf_field *f, double *rows_dev)
{
    const int rowlen = field_row_length(f);
    const size_t n = (size_t)f->ncell;
    nf_field::Geometry &g = f->geo;
    if (g.batch_steps != f->uv.nt) {
        NF_TRY(g.iVb.alloc(n * 4 * f->uv.nt));
        NF_TRY(g.absb.alloc(n * 2 * f->uv.nt));
        NF_TRY(g.zr.alloc((size_t)2 * f->uv.nt));
        // south slots of row 0 are never written (field.py:219): every step's planes start as zeros
        NF_HIP(hipMemsetAsync(g.iVb.get(), 0, sizeof(double) * n * 4 * f->uv.nt, f->stream));
        g.batch_steps = f->uv.nt;
        g.batch_version = -1;
    }
    if (g.batch_version != f->version) {  // scratch follows the weight set, z ranges follow the slab ownership
        NF_TRY(g.scratchb.alloc((size_t)std::max(f->ws.nrec, f->ws.nent) * f->uv.nt));
        std::vector<int> zr((size_t)2 * f->uv.nt);
        for (long t = 0; t < f->uv.nt; ++t) {
            const Levels lv = field_levels(f, t);
            zr[2 * t] = lv.z0;
            zr[2 * t + 1] = lv.z1;
        }
        NF_HIP(hipMemcpy(g.zr.get(), zr.data(), sizeof(int) * zr.size(), hipMemcpyHostToDevice));
        g.batch_version = f->version;
    }
    StepInput in;   // resident fields: step 0 is the base of all of them
    NF_TRY(field_step_input(f, 0, {0, (int)f->nz}, &in));
    FluxArgs a = flux_args(in);
    a.iV = g.iVb.get();
    a.absU = g.absb.get();
    a.absV = g.absb.get() + f->ncell;
    a.maxbits = g.maxbits.get();
    a.batch.nsteps = (int)f->uv.nt;
    a.batch.in_stride = f->nz * f->ncell;
    a.batch.zr = g.zr.get();
    NF_TRY(field_launch_flux(f, a));
    if (rowlen > 0) {
        NF_TRY(field_integral(f, g.iVb.get(), g.scratchb.get(), rows_dev, (int)f->uv.nt, (long)(4 * n), rowlen));
        NF_TRY(field_timed_k3_end(f));
    }
    // the resident single-step arrays keep their meaning: they hold the LAST step (what read_step returns)
    NF_HIP(hipMemcpyAsync(g.iV.get(), g.iVb.get() + (size_t)(f->uv.nt - 1) * 4 * n, sizeof(double) * 4 * n,
                          hipMemcpyDeviceToDevice, f->stream));
    NF_HIP(hipMemcpyAsync(g.abs.get(), g.absb.get() + (size_t)(f->uv.nt - 1) * 2 * n, sizeof(double) * 2 * n,
                          hipMemcpyDeviceToDevice, f->stream));
    f->derived_stale = false;
    return NF_OK;
}

extern "C" {

int nf_field_new(nf_field **self)
try {
    NF_REQUIRE(self, NF_ERR_ARG, "nf_field_new: null argument");
    *self = new nf_field();
    return NF_OK;
}
NF_API_CATCH
int nf_field_del(nf_field **self)
try {
    if (self && *self) {
        nf_field *f = *self;
        field_drop_events(f);
        field_drop_graph(f);
        delete f;
        *self = nullptr;
    }
    return NF_OK;
}
NF_API_CATCH
int nf_field_set_stream(nf_field **self, void *hip_stream)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_stream: null field");
    (*self)->stream = (hipStream_t)hip_stream;
    ++(*self)->version;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_bounds(nf_field **self, const void *bounds_lon, const void *bounds_lat, long ny, long nx,
                        int dtype, int on_device)
try {
    NF_REQUIRE(self && *self && bounds_lon && bounds_lat, NF_ERR_ARG, "nf_field_set_bounds: null argument");
    NF_REQUIRE(ny > 0 && nx > 0 && ny * nx < (1l << 31), NF_ERR_ARG, "nf_field_set_bounds: bad (ny, nx)");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_field_set_bounds: dtype must be NF_F64/NF_F32");
    NF_NEED_DEVICE();
    nf_field *f = *self;
    field_free_geometry(f);
    f->ny = ny;
    f->nx = nx;
    f->ncell = ny * nx;
    const size_t n = (size_t)f->ncell;
    nf_field::Geometry &g = f->geo;
    NF_TRY(g.xy.alloc(n * 8));
    NF_TRY(g.arc4.alloc(n * 4));
    NF_TRY(g.arcE.alloc(n));
    NF_TRY(g.arcN.alloc(n));
    NF_TRY(g.box.alloc(4));
    NF_TRY(g.iV.alloc(n * 4));
    NF_TRY(g.abs.alloc(n * 2));
    NF_TRY(g.maxbits.alloc(1));
    // field.py:59-63: the per-step arrays start as zeros (row 0's south slot stays zero for ever)
    NF_HIP(hipMemsetAsync(g.iV.get(), 0, sizeof(double) * n * 4, f->stream));
    NF_HIP(hipMemsetAsync(g.abs.get(), 0, sizeof(double) * n * 2, f->stream));
    NF_HIP(hipMemsetAsync(g.maxbits.get(), 0, sizeof(unsigned long long), f->stream));
    const size_t bytes = n * 4 * elem_size(dtype);
    DevArray<char> d_lon, d_lat;   // hipFree waits for the stream's work before releasing
    const void *plon = bounds_lon, *plat = bounds_lat;
    if (!on_device) {
        NF_TRY(d_lon.alloc(bytes));
        NF_TRY(d_lat.alloc(bytes));
        NF_HIP(hipMemcpyAsync(d_lon.get(), bounds_lon, bytes, hipMemcpyHostToDevice, f->stream));
        NF_HIP(hipMemcpyAsync(d_lat.get(), bounds_lat, bytes, hipMemcpyHostToDevice, f->stream));
        plon = d_lon.get();
        plat = d_lat.get();
    }
    NF_TRY(launch_geometry(plon, plat, dtype, f->ncell, g.xy.get(), g.arc4.get(), g.arcE.get(), g.arcN.get(), g.box.get(),
                           f->stream));
    unsigned long long keys[4] = {0, 0, 0, 0};
    NF_HIP(hipMemcpyAsync(keys, g.box.get(), sizeof keys, hipMemcpyDeviceToHost, f->stream));
    NF_HIP(hipStreamSynchronize(f->stream));
    for (int k = 0; k < 4; ++k) f->box[k] = box_key_to_double(keys[k]);
    f->grid_view.ncell = f->ncell;
    f->grid_view.d_xy = g.xy.get();
    f->grid_view.row_length = f->nx;  // (field_free_geometry above dropped the locator of the old corner table)
    ++f->grid_view.version;
    f->weights_built = false;
    ++f->version;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_thickness(nf_field **self, const double *thickness, long nz)
try {
    NF_REQUIRE(self && *self && thickness, NF_ERR_ARG, "nf_field_set_thickness: null argument");
    NF_REQUIRE(nz > 0 && nz < (1l << 30), NF_ERR_ARG, "nf_field_set_thickness: bad nz");
    NF_NEED_DEVICE();
    nf_field *f = *self;
    NF_TRY(f->thick.alloc((size_t)nz));
    NF_HIP(hipMemcpy(f->thick.get(), thickness, sizeof(double) * nz, hipMemcpyHostToDevice));
    f->nz = nz;
    ++f->version;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_uv(nf_field **self, const void *u, const void *v, long nt, int dtype, int on_device,
                    double fill_value)
try {
    NF_REQUIRE(self && *self && u && v, NF_ERR_ARG, "nf_field_set_uv: null argument");
    NF_REQUIRE(nt > 0, NF_ERR_ARG, "nf_field_set_uv: nt must be positive");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_field_set_uv: dtype must be NF_F64/NF_F32");
    nf_field *f = *self;
    f->uv.p[0] = u;
    f->uv.p[1] = v;
    f->uv.nt = nt;
    f->uv.dtype = dtype;
    f->uv.on_device = on_device;
    f->uv.fill = fill_value;
    ++f->version;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_missing_value(nf_field **self, double missing_value)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_missing_value: null field");
    (*self)->uv.fill2 = missing_value;
    ++(*self)->version;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_sverdrup(nf_field **self, int sverdrup)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_sverdrup: null field");
    (*self)->sverdrup = sverdrup ? 1 : 0;
    ++(*self)->version;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_compact(nf_field **self, int compact)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_compact: null field");
    nf_field *f = *self;
    if (!compact && f->geo.iV.get()) NF_TRY(field_ensure_derived(f));   // leaving the mode: the planes become whole again
    f->compact = compact ? 1 : 0;
    ++f->version;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_slab_range(nf_field **self, long s_begin, long s_end)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_slab_range: null field");
    NF_REQUIRE(s_begin >= 0 && s_end >= s_begin, NF_ERR_ARG, "nf_field_set_slab_range: need 0 <= begin <= end");
    (*self)->s_begin = s_begin;
    (*self)->s_end = s_end;
    ++(*self)->version;
    return NF_OK;
}
NF_API_CATCH

int nf_field_add_transect(nf_field **self, const double *xyz, int npts, int counterclock, int *transect_id)
try {
    NF_REQUIRE(self && *self && xyz, NF_ERR_ARG, "nf_field_add_transect: null argument");
    NF_REQUIRE(npts >= 2, NF_ERR_ARG, "nf_field_add_transect: need at least 2 points");
    nf_field *f = *self;
    f->polylines.emplace_back(xyz, xyz + 3 * (size_t)npts);
    f->poly_cc.push_back(counterclock ? 1 : 0);
    f->weights_built = false;
    if (transect_id) *transect_id = (int)f->polylines.size() - 1;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_unsupported_cells(nf_field **self, int skip)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_unsupported_cells: null field");
    NF_REQUIRE(skip == 0 || skip == 1, NF_ERR_ARG, "nf_field_set_unsupported_cells: policy must be 0 (refuse) or 1 (skip)");
    (*self)->skip_unsupported = skip;
    return NF_OK;
}
NF_API_CATCH

int nf_field_num_dropped_crossings(nf_field **self, size_t *n)
try {
    NF_REQUIRE(self && *self && n, NF_ERR_ARG, "nf_field_num_dropped_crossings: null argument");
    *n = (size_t)(*self)->ws.dropped;
    return NF_OK;
}
NF_API_CATCH
int nf_field_set_overlapping_cells(nf_field **self, int warn)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_overlapping_cells: null field");
    NF_REQUIRE(warn == 0 || warn == 1, NF_ERR_ARG, "nf_field_set_overlapping_cells: policy must be 0 (refuse) or 1 (warn)");
    (*self)->overlap_warn = warn;
    return NF_OK;
}
NF_API_CATCH

int nf_field_build_weights(nf_field **self, int numCellsPerBucket, double periodX)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_build_weights: null field");
    nf_field *f = *self;
    NF_REQUIRE(f->geo.xy.get(), NF_ERR_STATE, "nf_field_build_weights: set_bounds first");
    NF_REQUIRE(numCellsPerBucket > 0 && periodX >= 0.0, NF_ERR_ARG, "nf_field_build_weights: bad locator arguments");
    NF_NEED_DEVICE();
    std::vector<double> segs;
    std::vector<int> cc;
    f->tr_off.assign(1, 0);
    for (size_t p = 0; p < f->polylines.size(); ++p) {
        polyline_segments(f->polylines[p].data(), (int)(f->polylines[p].size() / 3), f->poly_cc[p], segs, cc);
        f->tr_off.push_back((int)cc.size());
    }
    f->weights_built = false;
    f->prof_scratch.reset();
    f->tprof_scratch.reset();
    f->area_scratch.reset();
    f->gross_scratch.reset();
    f->crossings.reset();
    f->class_scratch.reset();
    f->joint_table.reset();
    f->joint_flags.reset();
    f->joint_scratch.reset();
    const int bw = build_weights(f->geo.xy.get(), f->ncell, segs.data(), cc.data(), (int)cc.size(), periodX, &f->ws, f->stream,
                                 f->skip_unsupported, f->overlap_warn, nullptr, f->nx);
    if (bw != NF_OK) {
        // over-covered segment (overlapping cells): name the transect and its own segment index, not the batch's
        for (size_t q = 0; q < f->ws.coverage.size(); ++q)
            if ((long)q == (long)f->ws.over_seg) {
                size_t p = 0;
                while (p + 2 < f->tr_off.size() && (size_t)f->tr_off[p + 1] <= q) ++p;
                char buf[320];
                snprintf(buf, sizeof buf,
                         "nf_field_build_weights: transect %zu, target segment %zu is covered %.9g times by the cells of the "
                         "grid: cells overlap along it (a cell wrapped across the date line with periodX = 0, or duplicated "
                         "/ folded cells that are not identical), so part of the line would be counted twice",
                         p, q - (size_t)f->tr_off[p], f->ws.coverage[q]);
                set_error(buf);
                break;
            }
        return bw;
    }
    // the engine reduces its own planes: fold the (cell, edge) weights onto the unique edges of (eU, eV) (field.py:219-223)
    // (only on request -- nf_tuning_set("edge_weights", 1) -- because the records measure faster: see nf_integral.hip)
    if (integral_uses_edges()) NF_TRY(fold_weights(&f->ws, f->ncell, f->nx, f->stream));
    NF_TRY(f->tr_off_dev.alloc(f->tr_off.size()));
    NF_TRY(f->scratch.alloc((size_t)2 * std::max(f->ws.nrec, f->ws.nent)));
    NF_HIP(hipMemcpy(f->tr_off_dev.get(), f->tr_off.data(), sizeof(int) * f->tr_off.size(), hipMemcpyHostToDevice));
    f->weights_built = true;
    ++f->version;
    return NF_OK;
}
NF_API_CATCH

int nf_field_num_transects(nf_field **self, int *n)
try {
    NF_REQUIRE(self && *self && n, NF_ERR_ARG, "nf_field_num_transects: null argument");
    *n = (int)(*self)->polylines.size();
    return NF_OK;
}
NF_API_CATCH
int nf_field_num_segments(nf_field **self, int *nseg_total)
try {
    NF_REQUIRE(self && *self && nseg_total, NF_ERR_ARG, "nf_field_num_segments: null argument");
    NF_REQUIRE((*self)->weights_built, NF_ERR_STATE, "nf_field_num_segments: build_weights first");
    *nseg_total = (*self)->ws.nseg;
    return NF_OK;
}
NF_API_CATCH
int nf_field_segment_offsets(nf_field **self, int *offsets)
try {
    NF_REQUIRE(self && *self && offsets, NF_ERR_ARG, "nf_field_segment_offsets: null argument");
    NF_REQUIRE((*self)->weights_built, NF_ERR_STATE, "nf_field_segment_offsets: build_weights first");
    memcpy(offsets, (*self)->tr_off.data(), sizeof(int) * (*self)->tr_off.size());
    return NF_OK;
}
NF_API_CATCH
int nf_field_num_weights(nf_field **self, size_t *n)
try {
    NF_REQUIRE(self && *self && n, NF_ERR_ARG, "nf_field_num_weights: null argument");
    *n = (size_t)(*self)->ws.entries();
    return NF_OK;
}
NF_API_CATCH
int nf_field_get_weights(nf_field **self, int64_t *cell_edge, double *weight, int *seg_global)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_get_weights: null field");
    if ((*self)->ws.nrec == 0) return NF_OK;
    NF_NEED_DEVICE();
    return weights_to_host((*self)->ws, cell_edge, weight, seg_global);
}
NF_API_CATCH
int nf_field_get_coverage(nf_field **self, double *coverage)
try {
    NF_REQUIRE(self && *self && coverage, NF_ERR_ARG, "nf_field_get_coverage: null argument");
    NF_REQUIRE((*self)->weights_built || !(*self)->ws.coverage.empty(), NF_ERR_STATE,
               "nf_field_get_coverage: build_weights first");
    const std::vector<double> &c = (*self)->ws.coverage;
    if (!c.empty()) memcpy(coverage, c.data(), sizeof(double) * c.size());
    return NF_OK;
}
NF_API_CATCH
int nf_field_num_edge_weights(nf_field **self, size_t *n)
try {
    NF_REQUIRE(self && *self && n, NF_ERR_ARG, "nf_field_num_edge_weights: null argument");
    *n = (size_t)(*self)->ws.nent;
    return NF_OK;
}
NF_API_CATCH
int nf_field_get_edge_weights(nf_field **self, int *elem, int *seg_global, double *weight)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_get_edge_weights: null field");
    const WeightSet &ws = (*self)->ws;
    if (ws.nent == 0) return NF_OK;
    NF_NEED_DEVICE();
    std::vector<WeightSet::EdgeEntry> h((size_t)ws.nent);
    NF_HIP(hipMemcpy(h.data(), ws.ent.get(), sizeof(WeightSet::EdgeEntry) * h.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < h.size(); ++k) {   // pure re-indexing of the device result for the caller
        if (elem) elem[k] = h[k].elem;
        if (seg_global) seg_global[k] = h[k].seg;
        if (weight) weight[k] = h[k].w;
    }
    return NF_OK;
}
NF_API_CATCH
int nf_field_row_length(nf_field **self, int *n)
try {
    NF_REQUIRE(self && *self && n, NF_ERR_ARG, "nf_field_row_length: null argument");
    *n = field_row_length(*self);
    return NF_OK;
}
NF_API_CATCH

int nf_field_compute_flux(nf_field **self, long tIndex, double *row_host)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_compute_flux: null field");
    NF_NEED_DEVICE();
    nf_field *f = *self;
    const size_t n = f->weights_built ? field_row_length(f) : 0;   // no weights: the step alone, no row
    return field_sync(f, f->row, n, row_host, [&](double *row) { return field_step_async(f, tIndex, n > 0 ? row : nullptr); });
}
NF_API_CATCH

int nf_field_compute_all_async(nf_field **self, double *rows_dev)
try {
    NF_REQUIRE(self && *self && rows_dev, NF_ERR_ARG, "nf_field_compute_all_async: null argument");
    NF_NEED_DEVICE();
    nf_field *f = *self;
    NF_REQUIRE(f->weights_built, NF_ERR_STATE, "nf_field_compute_all_async: build_weights first");
    NF_TRY(field_cell_thick_current(f, "nf_field_compute_all_async"));   // before a capture, and for a rank that owns no step
    if (field_can_batch(f)) return field_all_steps_batched(f, rows_dev);
    NF_TRY(field_prepare_pass(f));   // allocations stay out of a graph capture
    // Replay a captured graph of the whole pass when nothing changed since it was captured.  Capture needs a real
    // (non-null) stream, resident fields (a cell thickness included), and no per-launch timing events.
    const bool can_graph =
        g_use_graph && f->stream != nullptr && f->uv.on_device && (!f->e3.p[0] || f->e3.on_device) && !f->timing;
    if (can_graph && f->graph_exec && f->graph_rows == rows_dev && f->graph_version == field_pass_version(f)) {
        NF_TRY(field_zero_unowned_rows(f, rows_dev));
        NF_HIP(hipGraphLaunch(f->graph_exec, f->stream));
        return NF_OK;
    }
    if (can_graph) {
        field_drop_graph(f);
        hipGraph_t graph = nullptr;
        if (hipStreamBeginCapture(f->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const int rc = field_all_steps_direct(f, rows_dev, false);
            hipError_t e = hipStreamEndCapture(f->stream, &graph);
            if (rc == NF_OK && e == hipSuccess && graph &&
                hipGraphInstantiate(&f->graph_exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                (void)hipGraphDestroy(graph);
                f->graph_rows = rows_dev;
                f->graph_version = field_pass_version(f);
                NF_TRY(field_zero_unowned_rows(f, rows_dev));
                NF_HIP(hipGraphLaunch(f->graph_exec, f->stream));
                return NF_OK;
            }
            if (graph) (void)hipGraphDestroy(graph);
            f->graph_exec = nullptr;
            (void)hipGetLastError();  // fall through to direct launches (they report any real error)
        } else {
            (void)hipGetLastError();
        }
    }
    return field_all_steps_direct(f, rows_dev);
}
NF_API_CATCH

int nf_field_compute_profile(nf_field **self, long tIndex, double *prof_host)
try {
    return field_product(self, kProfile, __func__, tIndex, 0, prof_host, true);
}
NF_API_CATCH

int nf_field_compute_profile_async(nf_field **self, long tIndex, double *prof_dev)
try {
    return field_product(self, kProfile, __func__, tIndex, 0, prof_dev, false);
}
NF_API_CATCH

int nf_field_set_tracer(nf_field **self, const void *tracer, long nt, int dtype, int on_device, double fill_value)
try {
    NF_REQUIRE(self && *self && tracer, NF_ERR_ARG, "nf_field_set_tracer: null argument");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_field_set_tracer: dtype must be NF_F64/NF_F32");
    nf_field *f = *self;
    NF_REQUIRE(f->uv.p[0] && f->uv.p[1], NF_ERR_STATE, "nf_field_set_tracer: set_uv first");
    NF_TRY(field_matches_uv(f, dtype, nt, "nf_field_set_tracer", "tracer", kCountSteps));
    f->tau.p[0] = tracer;
    f->tau.nt = nt;
    f->tau.dtype = dtype;
    f->tau.on_device = on_device ? 1 : 0;
    f->tau.fill = fill_value;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_tracer_missing_value(nf_field **self, double missing_value)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_tracer_missing_value: null field");
    (*self)->tau.fill2 = missing_value;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_tracer_reference(nf_field **self, double ref)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_tracer_reference: null field");
    NF_REQUIRE(std::isfinite(ref), NF_ERR_ARG, "nf_field_set_tracer_reference: the reference must be a finite number");
    (*self)->tau_ref = ref;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_tracer_wrap(nf_field **self, int wrap_x)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_tracer_wrap: null field");
    NF_REQUIRE(wrap_x == 0 || wrap_x == 1, NF_ERR_ARG, "nf_field_set_tracer_wrap: wrap_x must be 0 or 1");
    (*self)->tau_wrap = wrap_x;
    return NF_OK;
}
NF_API_CATCH

int nf_field_compute_tracer_flux(nf_field **self, long tIndex, double *row_host)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_compute_tracer_flux: null field");
    nf_field *f = *self;
    NF_REQUIRE(f->tau.p[0], NF_ERR_STATE, "nf_field_compute_tracer_flux: set_tracer first");
    NF_NEED_DEVICE();
    return field_sync(f, f->row, field_row_length(f), row_host,
                      [&](double *row) { return field_tracer_step_async(f, tIndex, row); });
}
NF_API_CATCH

int nf_field_compute_tracer_all_async(nf_field **self, double *rows_dev)
try {
    NF_REQUIRE(self && *self && rows_dev, NF_ERR_ARG, "nf_field_compute_tracer_all_async: null argument");
    nf_field *f = *self;
    NF_REQUIRE(f->tau.p[0], NF_ERR_STATE, "nf_field_compute_tracer_all_async: set_tracer first");
    NF_NEED_DEVICE();
    const int rowlen = field_row_length(f);
    for (long t = 0; t < f->uv.nt; ++t) NF_TRY(field_tracer_step_async(f, t, rows_dev + (size_t)t * rowlen));
    return NF_OK;
}
NF_API_CATCH

// the rules of one set of class edges; w prefixes the messages
static int class_edges_check(const std::string &w, const double *edges, int n)
{
    if (!(n >= 2 && n <= kMaxClassEdges)) {
        char buf[96];
        snprintf(buf, sizeof buf, "need 2 <= nedges <= %d, got %d", kMaxClassEdges, n);
        NF_REQUIRE(false, NF_ERR_ARG, w + buf);
    }
    for (int k = 0; k < n; ++k) {
        NF_REQUIRE(std::isfinite(edges[k]), NF_ERR_ARG, w + "every edge must be a finite number");
        NF_REQUIRE(k == 0 || edges[k] > edges[k - 1], NF_ERR_ARG, w + "the edges must be strictly increasing");
    }
    return NF_OK;
}

int nf_field_set_class_edges(nf_field **self, const double *edges, int nedges)
try {
    NF_REQUIRE(self && *self && edges, NF_ERR_ARG, "nf_field_set_class_edges: null argument");
    NF_TRY(class_edges_check("nf_field_set_class_edges: ", edges, nedges));
    nf_field *f = *self;
    f->class_edges.host.assign(edges, edges + nedges);
    f->class_edges.stale = true;
    return NF_OK;
}
NF_API_CATCH

int nf_field_compute_class_transport(nf_field **self, long tIndex, double *rows_host)
try {
    return field_product(self, kClassTransport, __func__, tIndex, 0, rows_host, true);
}
NF_API_CATCH

int nf_field_compute_class_transport_async(nf_field **self, long tIndex, double *rows_dev)
try {
    return field_product(self, kClassTransport, __func__, tIndex, 0, rows_dev, false);
}
NF_API_CATCH

int nf_field_compute_class_remap(nf_field **self, long tIndex, int carry, double *rows_host)
try {
    return field_product(self, kClassRemap, __func__, tIndex, carry, rows_host, true);
}
NF_API_CATCH

int nf_field_compute_class_remap_async(nf_field **self, long tIndex, int carry, double *rows_dev)
try {
    return field_product(self, kClassRemap, __func__, tIndex, carry, rows_dev, false);
}
NF_API_CATCH

int nf_field_set_depth_edges(nf_field **self, const double *edges, int nedges, double top)
try {
    NF_REQUIRE(self && *self && edges, NF_ERR_ARG, "nf_field_set_depth_edges: null argument");
    NF_TRY(class_edges_check("nf_field_set_depth_edges: ", edges, nedges));
    NF_REQUIRE(std::isfinite(top), NF_ERR_ARG, "nf_field_set_depth_edges: top must be a finite number");
    nf_field *f = *self;
    f->depth_edges.host.assign(edges, edges + nedges);
    f->depth_edges.stale = true;
    f->depth_top = top;
    return NF_OK;
}
NF_API_CATCH

int nf_field_compute_depth_transport(nf_field **self, long tIndex, int carry, double *rows_host)
try {
    return field_product(self, kDepthTransport, __func__, tIndex, carry, rows_host, true);
}
NF_API_CATCH

int nf_field_compute_depth_transport_async(nf_field **self, long tIndex, int carry, double *rows_dev)
try {
    return field_product(self, kDepthTransport, __func__, tIndex, carry, rows_dev, false);
}
NF_API_CATCH

int nf_field_set_depth_surfaces(nf_field **self, const void *const *surfaces, int m, long nt_s, int dtype, int on_device,
                                double fill_value, double top)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_depth_surfaces: null field");
    nf_field *f = *self;
    nf_field::Surfaces &sf = f->surf;
    if (!surfaces) {   // no surfaces; freeing the handle's buffers waits for the kernels that read them
        sf = nf_field::Surfaces{};
        return NF_OK;
    }
    NF_REQUIRE(m >= 1 && m <= kMaxSurfaces, NF_ERR_ARG, "nf_field_set_depth_surfaces: need 1 <= m <= 8 surfaces");
    for (int q = 0; q < m; ++q) NF_REQUIRE(surfaces[q], NF_ERR_ARG, "nf_field_set_depth_surfaces: null argument");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_field_set_depth_surfaces: dtype must be NF_F64/NF_F32");
    NF_REQUIRE(std::isfinite(top), NF_ERR_ARG, "nf_field_set_depth_surfaces: top must be a finite number");
    NF_REQUIRE(nt_s >= 1, NF_ERR_ARG, "nf_field_set_depth_surfaces: need nt_s = 1 (static) or the nt of uo/vo");
    NF_REQUIRE(f->uv.p[0] && f->uv.p[1], NF_ERR_STATE, "nf_field_set_depth_surfaces: set_uv first");
    NF_TRY(field_matches_uv(f, dtype, nt_s, "nf_field_set_depth_surfaces", "depth surfaces",
                            kStaticOk | kNameDtypes | kCountSteps));
    const bool upload = !on_device && nt_s == 1;   // a static host set: uploaded once, here
    DevArray<char> fixed;
    if (upload) {
        NF_REQUIRE(f->ncell > 0, NF_ERR_STATE, "nf_field_set_depth_surfaces: set_bounds first");
        NF_NEED_DEVICE();
        const size_t plane = (size_t)f->ncell * elem_size(dtype);
        NF_TRY(fixed.alloc(plane * m));
        for (int q = 0; q < m; ++q) NF_HIP(hipMemcpy(fixed.get() + (size_t)q * plane, surfaces[q], plane, hipMemcpyHostToDevice));
        NF_HIP(hipStreamSynchronize(f->stream));   // kernels in flight may still read the arrays these replace
    }
    sf.fixed = std::move(fixed);
    sf.fixed_ny = f->ny, sf.fixed_nx = f->nx;
    const size_t plane = (size_t)f->ncell * elem_size(dtype);
    for (int q = 0; q < kMaxSurfaces; ++q)
        sf.p[q] = q >= m ? nullptr : (upload ? (const void *)(sf.fixed.get() + (size_t)q * plane) : surfaces[q]);
    sf.m = m;
    sf.nt = nt_s;
    sf.dtype = dtype;
    sf.on_device = (on_device || upload) ? 1 : 0;
    sf.fill = fill_value;
    sf.top = top;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_depth_surfaces_missing_value(nf_field **self, double missing_value)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_depth_surfaces_missing_value: null field");
    (*self)->surf.fill2 = missing_value;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_depth_surfaces_wrap(nf_field **self, int wrap_x)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_depth_surfaces_wrap: null field");
    (*self)->surf.wrap = wrap_x ? 1 : 0;
    return NF_OK;
}
NF_API_CATCH

int nf_field_compute_surface_transport(nf_field **self, long tIndex, int carry, double *rows_host)
try {
    return field_product(self, kSurfaceTransport, __func__, tIndex, carry, rows_host, true);
}
NF_API_CATCH

int nf_field_compute_surface_transport_async(nf_field **self, long tIndex, int carry, double *rows_dev)
try {
    return field_product(self, kSurfaceTransport, __func__, tIndex, carry, rows_dev, false);
}
NF_API_CATCH

int nf_field_set_joint_class_edges(nf_field **self, const double *edges_a, int na, const double *edges_b, int nb)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_joint_class_edges: null field");
    nf_field *f = *self;
    if (!edges_a && !edges_b) {   // no joint classes
        f->joint_edges.host.clear();
        f->joint_na = f->joint_nb = 0;
        return NF_OK;
    }
    NF_REQUIRE(edges_a && edges_b, NF_ERR_ARG, "nf_field_set_joint_class_edges: null argument");
    NF_TRY(class_edges_check("nf_field_set_joint_class_edges: axis A: ", edges_a, na));
    NF_TRY(class_edges_check("nf_field_set_joint_class_edges: axis B: ", edges_b, nb));
    if ((na + 2) * (nb + 2) > kMaxJointRows) {
        char buf[200];
        snprintf(buf, sizeof buf, "nf_field_set_joint_class_edges: (na + 2) * (nb + 2) = %d joint rows, at most %d are supported",
                 (na + 2) * (nb + 2), kMaxJointRows);
        NF_REQUIRE(false, NF_ERR_ARG, buf);
    }
    f->joint_edges.host.assign(edges_a, edges_a + na);
    f->joint_edges.host.insert(f->joint_edges.host.end(), edges_b, edges_b + nb);
    f->joint_na = na;
    f->joint_nb = nb;
    f->joint_edges.stale = true;
    return NF_OK;
}
NF_API_CATCH

int nf_field_compute_joint_class_transport(nf_field **self, long tIndex, int carry, double *rows_host)
try {
    return field_product(self, kJointClassTransport, __func__, tIndex, carry, rows_host, true);
}
NF_API_CATCH

int nf_field_compute_joint_class_transport_async(nf_field **self, long tIndex, int carry, double *rows_dev)
try {
    return field_product(self, kJointClassTransport, __func__, tIndex, carry, rows_dev, false);
}
NF_API_CATCH

int nf_field_compute_tracer_profile(nf_field **self, long tIndex, double *prof_host)
try {
    return field_product(self, kTracerProfile, __func__, tIndex, 0, prof_host, true);
}
NF_API_CATCH

int nf_field_compute_tracer_profile_async(nf_field **self, long tIndex, double *prof_dev)
try {
    return field_product(self, kTracerProfile, __func__, tIndex, 0, prof_dev, false);
}
NF_API_CATCH

int nf_field_compute_area_profile(nf_field **self, long tIndex, double *rows_host)
try {
    return field_product(self, kAreaProfile, __func__, tIndex, 0, rows_host, true);
}
NF_API_CATCH

int nf_field_compute_area_profile_async(nf_field **self, long tIndex, double *rows_dev)
try {
    return field_product(self, kAreaProfile, __func__, tIndex, 0, rows_dev, false);
}
NF_API_CATCH

int nf_field_compute_gross_profile(nf_field **self, long tIndex, int carry, double *rows_host)
try {
    return field_product(self, kGrossProfile, __func__, tIndex, carry, rows_host, true);
}
NF_API_CATCH

int nf_field_compute_gross_profile_async(nf_field **self, long tIndex, int carry, double *rows_dev)
try {
    return field_product(self, kGrossProfile, __func__, tIndex, carry, rows_dev, false);
}
NF_API_CATCH

int nf_field_num_crossings(nf_field **self, size_t *n)
try {
    NF_REQUIRE(self && *self && n, NF_ERR_ARG, "nf_field_num_crossings: null argument");
    NF_REQUIRE((*self)->weights_built, NF_ERR_STATE, "nf_field_num_crossings: build_weights first");
    *n = (size_t)(*self)->ws.nrec;
    return NF_OK;
}
NF_API_CATCH

int nf_field_get_crossings(nf_field **self, int *seg_global, int64_t *cell, double *ta, double *tb)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_get_crossings: null field");
    NF_REQUIRE((*self)->weights_built, NF_ERR_STATE, "nf_field_get_crossings: build_weights first");
    // a one-off readback: three blocking copies, the cells widened on the host
    const WeightSet &ws = (*self)->ws;
    const size_t n = (size_t)ws.nrec;
    if (n == 0) return NF_OK;
    NF_REQUIRE(seg_global && cell && ta && tb, NF_ERR_ARG, "nf_field_get_crossings: null argument");
    NF_NEED_DEVICE();
    std::vector<int> c(n);
    std::vector<double> tab(2 * n);
    NF_HIP(hipMemcpy(seg_global, ws.seg.get(), sizeof(int) * n, hipMemcpyDeviceToHost));
    NF_HIP(hipMemcpy(c.data(), ws.cell.get(), sizeof(int) * n, hipMemcpyDeviceToHost));
    NF_HIP(hipMemcpy(tab.data(), ws.tab.get(), sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; ++k) cell[k] = c[k], ta[k] = tab[2 * k], tb[k] = tab[2 * k + 1];
    return NF_OK;
}
NF_API_CATCH

int nf_field_compute_crossings(nf_field **self, long tIndex, int carry, double *out_host)
try {
    return field_product(self, kCrossings, __func__, tIndex, carry, out_host, true);
}
NF_API_CATCH

int nf_field_compute_crossings_async(nf_field **self, long tIndex, int carry, double *out_dev)
try {
    return field_product(self, kCrossings, __func__, tIndex, carry, out_dev, false);
}
NF_API_CATCH

int nf_field_compute_gross_class_transport(nf_field **self, long tIndex, int carry, double *rows_host)
try {
    return field_product(self, kGrossClassTransport, __func__, tIndex, carry, rows_host, true);
}
NF_API_CATCH

int nf_field_compute_gross_class_transport_async(nf_field **self, long tIndex, int carry, double *rows_dev)
try {
    return field_product(self, kGrossClassTransport, __func__, tIndex, carry, rows_dev, false);
}
NF_API_CATCH

int nf_field_compute_gross_class_remap(nf_field **self, long tIndex, int carry, double *rows_host)
try {
    return field_product(self, kGrossClassRemap, __func__, tIndex, carry, rows_host, true);
}
NF_API_CATCH

int nf_field_compute_gross_class_remap_async(nf_field **self, long tIndex, int carry, double *rows_dev)
try {
    return field_product(self, kGrossClassRemap, __func__, tIndex, carry, rows_dev, false);
}
NF_API_CATCH

int nf_field_compute_class_area(nf_field **self, long tIndex, double *rows_host)
try {
    return field_product(self, kClassArea, __func__, tIndex, 0, rows_host, true);
}
NF_API_CATCH

int nf_field_compute_class_area_async(nf_field **self, long tIndex, double *rows_dev)
try {
    return field_product(self, kClassArea, __func__, tIndex, 0, rows_dev, false);
}
NF_API_CATCH

int nf_field_set_class_tracer(nf_field **self, const void *tracer, long nt, int dtype, int on_device, double fill_value)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_class_tracer: null field");
    nf_field *f = *self;
    if (!tracer) {   // back to "the class field is the carried tracer"
        f->sig.p[0] = nullptr;
        f->sig.nt = 0;
        f->sig.fill = f->sig.fill2 = std::numeric_limits<double>::quiet_NaN();
        return NF_OK;
    }
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_field_set_class_tracer: dtype must be NF_F64/NF_F32");
    NF_REQUIRE(f->uv.p[0] && f->uv.p[1], NF_ERR_STATE, "nf_field_set_class_tracer: set_uv first");
    NF_TRY(field_matches_uv(f, dtype, nt, "nf_field_set_class_tracer", "class tracer", kNameDtypes | kCountSteps));
    f->sig.p[0] = tracer;
    f->sig.nt = nt;
    f->sig.dtype = dtype;
    f->sig.on_device = on_device ? 1 : 0;
    f->sig.fill = fill_value;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_class_tracer_missing_value(nf_field **self, double missing_value)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_class_tracer_missing_value: null field");
    (*self)->sig.fill2 = missing_value;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_cell_thickness(nf_field **self, const void *e3u, const void *e3v, long nt_th, int dtype, int on_device,
                                double fill_value)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_cell_thickness: null field");
    nf_field *f = *self;
    if (!e3u) {   // back to the per-level thickness
        f->e3.p[0] = f->e3.p[1] = nullptr;
        f->e3.nt = 0;
        f->e3.fill = f->e3.fill2 = std::numeric_limits<double>::quiet_NaN();
        f->e3u_static.reset(), f->e3v_static.reset(), f->e3.stage[0].reset(), f->e3.stage[1].reset();
        ++f->version;
        return NF_OK;
    }
    NF_REQUIRE(e3v, NF_ERR_ARG, "nf_field_set_cell_thickness: e3v is null (both arrays or neither)");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_field_set_cell_thickness: dtype must be NF_F64/NF_F32");
    NF_REQUIRE(f->uv.p[0] && f->uv.p[1], NF_ERR_STATE, "nf_field_set_cell_thickness: set_uv and set_thickness first");
    NF_TRY(field_matches_uv(f, dtype, nt_th, "nf_field_set_cell_thickness", "cell thickness",
                            kStaticOk | kNameDtypes | kCountSteps));
    NF_REQUIRE(f->thick.get(), NF_ERR_STATE, "nf_field_set_cell_thickness: set_thickness first (it fixes nz)");
    const bool upload = !on_device && nt_th == 1;   // a static host array: uploaded once, here
    if (upload) {
        NF_REQUIRE(f->ncell > 0, NF_ERR_STATE, "nf_field_set_cell_thickness: set_bounds first");
        NF_NEED_DEVICE();
        const size_t bytes = (size_t)f->nz * f->ncell * elem_size(dtype);
        DevArray<char> du, dv;
        NF_TRY(du.alloc(bytes));
        NF_TRY(dv.alloc(bytes));
        NF_HIP(hipMemcpy(du.get(), e3u, bytes, hipMemcpyHostToDevice));
        NF_HIP(hipMemcpy(dv.get(), e3v, bytes, hipMemcpyHostToDevice));
        NF_HIP(hipStreamSynchronize(f->stream));   // kernels in flight may still read the arrays these replace
        f->e3u_static = std::move(du);
        f->e3v_static = std::move(dv);
        f->e3_static_nz = f->nz, f->e3_static_ny = f->ny, f->e3_static_nx = f->nx;
        e3u = f->e3u_static.get();
        e3v = f->e3v_static.get();
    } else {
        f->e3u_static.reset(), f->e3v_static.reset();
    }
    f->e3.p[0] = e3u;
    f->e3.p[1] = e3v;
    f->e3.nt = nt_th;
    f->e3.dtype = dtype;
    f->e3.on_device = (on_device || upload) ? 1 : 0;
    f->e3.fill = fill_value;
    ++f->version;
    return NF_OK;
}
NF_API_CATCH

int nf_field_set_cell_thickness_missing_value(nf_field **self, double missing_value)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_set_cell_thickness_missing_value: null field");
    (*self)->e3.fill2 = missing_value;
    ++(*self)->version;
    return NF_OK;
}
NF_API_CATCH

int nf_field_compute_class_tracer_transport(nf_field **self, long tIndex, double *rows_host)
try {
    return field_product(self, kClassTracerTransport, __func__, tIndex, 0, rows_host, true);
}
NF_API_CATCH

int nf_field_compute_class_tracer_transport_async(nf_field **self, long tIndex, double *rows_dev)
try {
    return field_product(self, kClassTracerTransport, __func__, tIndex, 0, rows_dev, false);
}
NF_API_CATCH

int nf_field_read_step(nf_field **self, double *iV_host, double *eU_host, double *eV_host, double *max_abs)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_read_step: null field");
    nf_field *f = *self;
    nf_field::Geometry &g = f->geo;
    NF_REQUIRE(g.iV.get(), NF_ERR_STATE, "nf_field_read_step: set_bounds first");
    NF_NEED_DEVICE();
    if (iV_host || eU_host || eV_host) NF_TRY(field_ensure_derived(f));
    const size_t n = (size_t)f->ncell;
    if (iV_host) {  // re-pack the planes into the reference's (ncell,4) layout, then one D2H into the caller's array
        NF_TRY(g.aos.reserve(n * 4));
        NF_TRY(launch_planes_to_aos(g.iV.get(), f->ncell, g.aos.get(), f->stream));
        NF_HIP(hipMemcpyAsync(iV_host, g.aos.get(), sizeof(double) * n * 4, hipMemcpyDeviceToHost, f->stream));
    }
    if (eU_host) NF_HIP(hipMemcpyAsync(eU_host, g.abs.get(), sizeof(double) * n, hipMemcpyDeviceToHost, f->stream));
    if (eV_host) NF_HIP(hipMemcpyAsync(eV_host, g.abs.get() + n, sizeof(double) * n, hipMemcpyDeviceToHost, f->stream));
    if (max_abs) {
        unsigned long long b = 0;
        NF_HIP(hipMemcpyAsync(&b, g.maxbits.get(), sizeof b, hipMemcpyDeviceToHost, f->stream));
        NF_HIP(hipStreamSynchronize(f->stream));
        memcpy(max_abs, &b, 8);
    }
    NF_HIP(hipStreamSynchronize(f->stream));
    return NF_OK;
}
NF_API_CATCH

int nf_field_reset_max(nf_field **self)
try {
    NF_REQUIRE(self && *self && (*self)->geo.maxbits.get(), NF_ERR_STATE, "nf_field_reset_max: set_bounds first");
    NF_HIP(hipMemsetAsync((*self)->geo.maxbits.get(), 0, sizeof(unsigned long long), (*self)->stream));
    return NF_OK;
}
NF_API_CATCH

int nf_field_get_arclengths(nf_field **self, double *arc_host)
try {
    NF_REQUIRE(self && *self && arc_host, NF_ERR_ARG, "nf_field_get_arclengths: null argument");
    NF_REQUIRE((*self)->geo.arc4.get(), NF_ERR_STATE, "nf_field_get_arclengths: set_bounds first");
    NF_HIP(hipMemcpy(arc_host, (*self)->geo.arc4.get(), sizeof(double) * 4 * (size_t)(*self)->ncell, hipMemcpyDeviceToHost));
    return NF_OK;
}
NF_API_CATCH

int nf_field_get_points(nf_field **self, double *points_host)
try {
    NF_REQUIRE(self && *self && points_host, NF_ERR_ARG, "nf_field_get_points: null argument");
    nf_field *f = *self;
    NF_REQUIRE(f->geo.xy.get(), NF_ERR_STATE, "nf_field_get_points: set_bounds first");
    DevArray<double> points;
    NF_TRY(points.alloc(12 * (size_t)f->ncell));
    NF_TRY(launch_points_from_corner_table(f->geo.xy.get(), f->ncell, points.get(), f->stream));
    NF_HIP(hipMemcpyAsync(points_host, points.get(), sizeof(double) * 12 * (size_t)f->ncell, hipMemcpyDeviceToHost,
                          f->stream));
    NF_HIP(hipStreamSynchronize(f->stream));
    return NF_OK;
}
NF_API_CATCH

int nf_field_get_box(nf_field **self, double *lonmin, double *lonmax, double *latmin, double *latmax)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_get_box: null field");
    NF_REQUIRE(lonmin && lonmax && latmin && latmax, NF_ERR_ARG, "nf_field_get_box: null argument");
    NF_REQUIRE((*self)->geo.xy.get(), NF_ERR_STATE, "nf_field_get_box: set_bounds first");
    *lonmin = (*self)->box[0];
    *lonmax = (*self)->box[1];
    *latmin = (*self)->box[2];
    *latmax = (*self)->box[3];
    return NF_OK;
}
NF_API_CATCH

int nf_field_device_ptr(nf_field **self, int which, void **dev)
try {
    NF_REQUIRE(self && *self && dev, NF_ERR_ARG, "nf_field_device_ptr: null argument");
    nf_field *f = *self;
    if (which >= 0 && which <= 2) NF_TRY(field_ensure_derived(f));   // compact mode: the derived planes on demand
    switch (which) {
        case 0: *dev = f->geo.iV.get(); break;
        case 1: *dev = f->geo.abs.get(); break;
        case 2: *dev = f->geo.abs.get() ? f->geo.abs.get() + f->ncell : nullptr; break;
        case 3: *dev = f->geo.arc4.get(); break;
        case 4: *dev = f->geo.xy.get(); break;
        default: NF_REQUIRE(false, NF_ERR_ARG, "nf_field_device_ptr: unknown array id");
    }
    return NF_OK;
}
NF_API_CATCH

int nf_field_grid(nf_field **self, Grid_t **grid)
try {
    NF_REQUIRE(self && *self && grid, NF_ERR_ARG, "nf_field_grid: null argument");
    NF_REQUIRE((*self)->geo.xy.get(), NF_ERR_STATE, "nf_field_grid: set_bounds first");
    *grid = &(*self)->grid_view;
    return NF_OK;
}
NF_API_CATCH

int nf_field_timing(nf_field **self, int enable)
try {
    NF_REQUIRE(self && *self, NF_ERR_ARG, "nf_field_timing: null field");
    nf_field *f = *self;
    if (!enable) field_drop_events(f);
    f->ev_used = 0;
    f->ev_dropped = 0;
    f->timing = enable != 0;
    if (enable > 1) NF_TRY(field_reserve_events(f, (size_t)enable));   // event creation stays out of the timed region
    ++f->version;
    return NF_OK;
}
NF_API_CATCH
int nf_field_timing_read(nf_field **self, long *launches, double *total_ms)
try {
    NF_REQUIRE(self && *self && launches && total_ms, NF_ERR_ARG, "nf_field_timing_read: null argument");
    nf_field *f = *self;
    NF_HIP(hipStreamSynchronize(f->stream));
    double tot = 0.0, flux = 0.0, expand = 0.0, k3 = 0.0;
    for (size_t k = 0; k < f->ev_used; ++k) {
        const auto &t = f->ev[k];
        float ms = 0.f, part = 0.f;
        if (t.has_k3) {
            NF_HIP(hipEventElapsedTime(&part, t.e1, t.e2));
            k3 += part;
            part = 0.f;
        }
        NF_HIP(hipEventElapsedTime(&ms, t.e0, t.e1));
        tot += ms;
        if (t.has_mid) {
            NF_HIP(hipEventElapsedTime(&part, t.e0, t.mid));
            flux += part;
            expand += ms - part;
        } else {
            flux += ms;
        }
    }
    *launches = (long)f->ev_used;
    *total_ms = tot;
    f->last_flux_ms = flux;
    f->last_expand_ms = expand;
    f->last_k3_ms = k3;
    f->ev_used = 0;
    return NF_OK;
}
NF_API_CATCH
int nf_field_timing_split(nf_field **self, double *flux_ms, double *expand_ms)
try {
    NF_REQUIRE(self && *self && flux_ms && expand_ms, NF_ERR_ARG, "nf_field_timing_split: null argument");
    *flux_ms = (*self)->last_flux_ms;
    *expand_ms = (*self)->last_expand_ms;
    return NF_OK;
}
NF_API_CATCH
int nf_field_timing_k3(nf_field **self, double *k3_ms)
try {
    NF_REQUIRE(self && *self && k3_ms, NF_ERR_ARG, "nf_field_timing_k3: null argument");
    *k3_ms = (*self)->last_k3_ms;
    return NF_OK;
}
NF_API_CATCH

}  // extern "C"
