// nf_common.h -- shared declarations of the gfx950 transect-flux engine (internal; the public surface is
// include/nemoflux_amd.h).  Written for CDNA4 only: 64-lane wavefronts, 256 CUs in 8 XCDs.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <string>
#include <cmath>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "../../include/nemoflux_amd.h"

namespace nf {

// [flux-fingerprint-begin]  (bench.flux_source_sha16 hashes nf_flux.hip and the marked parts of this header: what K1 is built from)
constexpr int kWave = 64;        // CDNA wavefront
constexpr int kBlock = 256;      // 4 waves per workgroup
constexpr int kXcds = 8;         // MI355X: 8 XCDs, workgroups are dealt round-robin over them
constexpr double kDeg2Rad = 3.14159265358979323846 / 180.0;  // geo.py:4
constexpr double kEarthRadiusSv = 6371000.0;                 // field.py:12
// [flux-fingerprint-end]

void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define NF_HIP(call)                                                   \
    do {                                                               \
        hipError_t e_ = (call);                                        \
        if (e_ != hipSuccess) return nf::hip_fail(e_, #call, __FILE__, __LINE__); \
    } while (0)

#define NF_REQUIRE(cond, code, msg)            \
    do {                                       \
        if (!(cond)) {                         \
            nf::set_error(msg);                \
            return (code);                     \
        }                                      \
    } while (0)

#define NF_TRY(call)                  \
    do {                              \
        int rc_ = (call);             \
        if (rc_ != NF_OK) return rc_; \
    } while (0)

// [flux-fingerprint-begin]
// ---- XCD-aware tile mapping -------------------------------------------------------------------------
// Workgroup b lands on XCD b % 8.  Give every XCD one CONTIGUOUS band of logical tiles so that (a) the
// neighbour-slot stores of the edge-flux kernel (row j -> row j+1, column i -> i+1) meet the owning row's
// stores in the SAME L2 and leave it as whole lines, and (b) each L2 streams one band of every slab.
// Grid must be launched with xcd_grid(ntiles) workgroups; tiles >= ntiles exit.
__host__ __device__ inline unsigned xcd_grid(unsigned ntiles) { return ((ntiles + kXcds - 1) / kXcds) * kXcds; }
__device__ inline unsigned xcd_tile(unsigned b, unsigned grid) { return (b % kXcds) * (grid / kXcds) + b / kXcds; }
// [flux-fingerprint-end]

// ---- cells the weights / the point location are not defined on (docs/PARITY.md) --------------------------------
// v = (x0,y0,...,x3,y3) of a quad in the (lon,lat) plane
__device__ inline bool quad_is_nonconvex(const double *v)
{
    // a corner AT a geographic pole that is not the end of an edge lying on the pole line (|lat| = 90 along a whole edge,
    // as in the top row of an un-rotated lon-lat grid, is fine): the pole's longitude is arbitrary, so the planar quad is
    // not the image of the cell, convex or not
    int npole = 0, first = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (fabs(v[2 * k + 1]) >= 90.0 - 1.e-9) {
            ++npole;
            if (first < 0) first = k;
        }
    if (npole == 1 || npole == 3) return true;
    if (npole == 2 && !(fabs(v[2 * ((first + 1) & 3) + 1]) >= 90.0 - 1.e-9 || (first == 0 && fabs(v[2 * 3 + 1]) >= 90.0 - 1.e-9)))
        return true;   // opposite corners
    // a geographic pole INSIDE the cell (a rotated grid whose pole is not a mesh node): going round the four corners the
    // longitude winds once around the globe -- the differences, each taken the short way, add up to +-360 instead of 0 --
    // and the planar quad is a sliver along the pole line, not the image of the cell
    double turn = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double d = v[2 * ((k + 1) & 3)] - v[2 * k];
        d -= 360.0 * rint(d / 360.0);
        turn += d;
    }
    if (fabs(turn) > 180.0) return true;
    double cmin = 0.0, cmax = 0.0, scale = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3, k2 = (k + 2) & 3;
        const double ex = v[2 * k1] - v[2 * k], ey = v[2 * k1 + 1] - v[2 * k + 1];
        const double fx = v[2 * k2] - v[2 * k1], fy = v[2 * k2 + 1] - v[2 * k1 + 1];
        const double cr = ex * fy - ey * fx;
        cmin = fmin(cmin, cr);
        cmax = fmax(cmax, cr);
        scale = fmax(scale, ex * ex + ey * ey);
    }
    return cmin < -1.e-12 * scale && cmax > 1.e-12 * scale;
}


// ---- date-line unwrap (round 4) -----------------------------------------------------------------------------------------
// A global file stores bounds_lon wrapped into one period (say [-180,180]), so the cell that straddles the cut has corners
// ~350 degrees apart: as a planar quad it is a clockwise sliver across the whole domain that the clip would accept and count
// a second time.  With a periodic locator (periodX > 0) every corner is brought to within periodX/2 of corner 0 in the
// lane's REGISTER copy of the cell -- the rule the reference's own generator applies to its rotated grids
// (datagen.py:161-166, with 270 degrees there).  The corner table in HBM, getPoints() and the arc lengths keep the file's
// values.  mint's own behaviour on such cells is parity unpinned.
__device__ inline void unwrap_quad(double *v, double periodX)
{
    if (!(periodX > 0.0)) return;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const double n = rint((v[2 * k] - v[0]) / periodX);
        if (n != 0.0) v[2 * k] -= n * periodX;
    }
}
// a cell with a corner that is not a finite number (NaN or infinite bounds on land-only subdomains) is no cell at all: it
// takes part in nothing and the coverage of a line through it says so
__device__ inline bool quad_is_finite(const double *v)
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) ok = ok && (fabs(v[k]) <= 1.7976931348623157e308);
    return ok;
}
// A target segment covered more than once is counted twice somewhere (overlapping cells): an error.  Two conditions, both
// needed (round-4 advisor): the excess in the segment's parameter, cov - 1 > kCoverTol, AND the same excess as a LENGTH,
// (cov - 1) |d| > kCoverLenTol max(1, |coordinates|) degrees.  The parameter of a sub-segment end carries a rounding error of
// about eps |coordinates| / |d|: on a target segment of 1e-9 degrees across a cell edge that is 1e-6 in t -- the two cells'
// pieces then no longer match within kTolT and the shared stretch counts twice, an excess of up to 5e-7 in t but 1e-15
// degrees of line.  Real overlaps (a date-line cell with periodX = 0, duplicated cells) double whole cell crossings.
constexpr double kCoverTol = 1.e-8;
constexpr double kCoverLenTol = 1.e-9;
inline bool over_covered(double cov, const double *seg4 /* x0, y0, dx, dy */)
{
    if (!(cov > 1.0 + kCoverTol)) return false;
    const double len = std::sqrt(seg4[2] * seg4[2] + seg4[3] * seg4[3]);
    double m = 1.0;
    for (double c : {seg4[0], seg4[1], seg4[0] + seg4[2], seg4[1] + seg4[3]}) m = std::fabs(c) > m ? std::fabs(c) : m;
    return (cov - 1.0) * len > kCoverLenTol * m;
}

// ---- launchers (defined in the .hip files) ----------------------------------------------------------
// K0: geometry.  bounds (ncell,4) of T -> corner table xy (ncell,4,2), arc (ncell,4), arcE/arcN (ncell),
// lon/lat box (4 doubles: lonmin, lonmax, latmin, latmax as order-preserving keys; see nf_geom.hip).
int launch_geometry(const void *blon, const void *blat, int dtype, long ncell, double *xy, double *arc4,
                    double *arcE, double *arcN, unsigned long long *box_keys, hipStream_t s);
int launch_corner_table_from_points(const double *points, long ncell, double *xy, hipStream_t s);
int launch_points_from_corner_table(const double *xy, long ncell, double *points, hipStream_t s);
double box_key_to_double(unsigned long long k);

// [flux-fingerprint-begin]
// several time steps in one launch (launch-bound small grids): step tb reads u,v + tb*in_stride, integrates levels
// [zr[2tb], zr[2tb+1]) and writes planes iV + tb*4*ncell, abs + tb*2*ncell.  zr == nullptr: one step (z0, z1).
struct StepBatch {
    int nsteps = 0;
    long in_stride = 0;       // elements of the field dtype between consecutive time steps
    const int *zr = nullptr;  // device, 2*nsteps
};

// K1: vertical integral of one time step's slabs [z0,z1) + edge fluxes (the bandwidth-bound kernel).
struct FluxArgs {
    const void *u, *v;        // base of the time step: (nz, ncell)
    int dtype;                // NF_F64 / NF_F32
    long ncell, ny, nx;
    int z0, z1;
    const double *thickness;  // device, nz
    const double *arcE, *arcN;
    double fill;              // NaN = none
    double fill2 = __builtin_nan("");   // a second missing marker (CF missing_value that differs from _FillValue); NaN = none
    double scale;             // 1 or 6371000/1e6
    int sverdrup;
    double *iV, *absU, *absV; // resident outputs
    unsigned long long *maxbits;  // running max as the bits of a non-negative double
    StepBatch batch;
    int signed_only = 0;      // 1: store only planes 1 (eU) and 2 (eV); launch_expand_planes derives the other four
    // 1 (with signed_only): iV is ONE stream E of 2 * ncell doubles, E[2c] = eU[c], E[2c + 1] = eV[c], and nothing else is
    // stored (an inner step of a per-step pass, read by the pair form of K3 only); needs flux_supports_interleaved
    int interleaved = 0;
    // timing: when the default step runs as flux kernel + expansion, mid_event is recorded between the two launches
    hipEvent_t mid_event = nullptr;
    bool *mid_recorded = nullptr;
};
int launch_flux(const FluxArgs &a, hipStream_t s);
bool flux_supports_signed_only(const FluxArgs &a);
// the interleaved store form: the signed-only form's conditions, and a launch that the two-field kernel takes (the one-field
// form of small launches has eU and eV in different wavefronts)
bool flux_supports_interleaved(const FluxArgs &a);
// planes 0 (south copies), 3 (west copies incl. the periodic wrap) and |eU|, |eV| from planes 1 and 2 (field.py:209-232)
int launch_expand_planes(double *iV, double *absUV, long ncell, long ny, long nx, hipStream_t s);
int tuning_set(const char *name, int value);
long tuning_version();
int launch_planes_to_aos(const double *planes, long ncell, double *aos, hipStream_t s);
// [flux-fingerprint-end]

// The one owner of a device allocation: a pointer and its element count, freed by the destructor (hipFree waits for the
// device).  Move-only.  size() == 0 means nothing is held -- also after a failed allocation, so the next call tries again.
template <typename T>
class DevArray {
public:
    DevArray() = default;
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
    DevArray(DevArray &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DevArray &operator=(DevArray &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~DevArray() { reset(); }
    // free, then allocate exactly n elements (n == 0: one element, at least 16 bytes)
    int alloc(size_t n)
    {
        reset();
        void *q = nullptr;
        NF_HIP(hipMalloc(&q, n ? sizeof(T) * n : (sizeof(T) > 16 ? sizeof(T) : 16)));
        p_ = static_cast<T *>(q);
        n_ = n ? n : 1;
        return NF_OK;
    }
    // grow only: re-allocates (the contents are lost) when fewer than n elements are held; *grown says whether it did
    int reserve(size_t n, bool *grown = nullptr)
    {
        const bool g = n_ == 0 || n_ < n;
        if (grown) *grown = g;
        return g ? alloc(n) : NF_OK;
    }
    void reset()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr, n_ = 0;
    }
    T *get() const { return p_; }
    size_t size() const { return n_; }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

// K2: batched polyline weights.
struct WeightSet {  // device-resident result: one record per (target segment, crossed cell), sorted by segment, ta
    long nrec = 0;
    DevArray<int> cell;        // cell id of the record
    DevArray<double> w4;       // 4 edge weights per record (S,E,N,W), multiplicity applied
    DevArray<int> seg;         // global segment id of the record
    DevArray<double> tab;      // (ta, tb) per record: the piece's parameters on its own target segment (the crossings)
    int nseg = 0;              // total target segments
    DevArray<int> seg_start;   // (nseg+1) CSR over records
    // host: fraction of every target segment that lies inside cells of the grid (sum of coef*(tb-ta) over its records);
    // 1 = inside the grid, each point counted once; < 1 = part of the segment is outside (contributes 0, like mint)
    std::vector<double> coverage;
    int over_seg = -1;         // first target segment build_weights found covered more than once (over_covered), or -1
    long dropped = 0;          // skip policy: (cell, segment image) crossings of unsupported cells that were left out
    // Unique-edge form for the engine's own planes (fold_weights): the south / west slots of integratedVelocity are copies
    // of the neighbours' north / east values (field.py:219-223), so every (cell, edge) weight is folded onto the element
    // of the two signed planes that really carries it and duplicates are merged per target segment (adjacent cells
    // share an edge): about half as many entries as 4 per record, ONE gather each.
    struct EdgeEntry {
        int elem;   // index into [eU | eV] = planes 1 and 2 taken as one array of 2*ncell values
        int seg;    // global target segment
        double w;   // summed weight
    };
    long nent = 0;
    DevArray<EdgeEntry> ent;     // sorted by (segment, elem)
    DevArray<int> ent_start;     // (nseg+1) CSR over entries
    long entries() const { return 4 * nrec; }  // mint's view: (cell*4+edge, weight) entries
    void release() { *this = WeightSet(); }
};
// builds ws.ent / ws.ent_start from the records, for a grid of nx columns (row-0 south slots carry no flux: dropped)
int fold_weights(WeightSet *ws, long ncell, long nx, hipStream_t s);
// expands records into mint-style entries (host arrays): cell_edge = cell*4+edge, weight, seg
int weights_to_host(const WeightSet &ws, int64_t *cell_edge, double *weight, int *seg);
// segs_host: (nseg,4) = x0,y0,dx,dy ; seg_cc_host: counterclock flag per segment
// skip_unsupported: 0 = a target segment that overlaps a non-convex / pole-vertex cell is an error (default); 1 = such
// cells contribute nothing and the segment's coverage is < 1
// The locator of a grid (nf_weights.hip: bounding boxes of the cells and of groups of 16, 256, ... consecutive cells) for one
// period, kept by whoever owns the corner table -- mint's buildLocator builds it once per PolylineIntegral; here a Grid_t keeps
// it for all the PolylineIntegral objects made on it (fluxviz / fluxplot make one per transect).  build_weights fills it when
// it does not match the grid it is called with.
struct Box4;   // nf_locator.h
struct LocatorBoxes {
    std::vector<DevArray<Box4>> level;   // level[l]: the boxes of level l (0 = cells)
    std::vector<long> count;
    const double *xy = nullptr;  // the corner table the boxes were built from
    long ncell = 0;
    double period = -1.0;
    // Objects that share a Grid share this cache.  Whoever may (re)build it or walks it holds `mtx` for the whole call
    // (computeWeights / findPoints are synchronous: the kernels that read the boxes have finished when the call returns), and
    // so does whoever releases it (new points, new row length, grid deletion): two host threads driving their own
    // PolylineIntegral objects on one Grid are serialised here instead of racing on release() (round-5 advisor).
    std::mutex mtx;
    void release();
};
// overlap_warn: 0 = a target segment covered more than once (over_covered) is an error (default); 1 = the build goes through,
// out->over_seg names the first such segment and the coverage says how much (the caller warns)
// boxes: nullptr = the locator lives for this build only (the batched build of a Field)
// row_length: the cells are rows of this many (a Field's (ny, nx) grid: the locator groups them in 4 x 4 blocks); 0 = unknown
int build_weights(const double *xy, long ncell, const double *segs_host, const int *seg_cc_host, int nseg,
                  double periodX, WeightSet *out, hipStream_t s, int skip_unsupported = 0, int overlap_warn = 0,
                  LocatorBoxes *boxes = nullptr, long row_length = 0);
// gives the idle scratch memory that weight builds / point searches keep between calls (a process-wide pool of at most 4
// scratches of at most 1 GiB each) back to the system
void weights_trim_scratch();

struct Transects {   // the transect side of K3: the records of all target segments, and the segments of every transect
    const WeightSet *ws = nullptr;
    const int *tr_offsets_dev = nullptr;   // device, (ntransect + 1) segment offsets
    int ntransect = 0;
    long row_length() const { return ws->nseg + ntransect; }   // a row: [ per-segment sums | per-transect sums ]
};

// K3: gather + wavefront segmented reduction -> per-segment sums, then per-transect sums.
// row: (nseg + ntransect) doubles in HBM; tr_offsets_dev: (ntransect+1) segment offsets.
// scratch: at least ws.nrec doubles.
// data: (ncell,4) AoS (planes = 0), [4][ncell] planes (planes = 1), or the engine's own planes read through their two
// signed members only (planes = 2; needs nx for the neighbour indexing).
// nsteps > 1: step tb gathers from data + tb*data_stride and writes row + tb*row_stride (scratch: nsteps*ws.nrec).
// planes = 2 uses the unique-edge entries when fold_weights built them (scratch: nsteps * max(ws.nrec, ws.nent)).
// rec_cells: the row of data each record reads (nullptr = ws.cell; a Level-1 object's rows gathered per record: 0..nrec-1).
void integral_use_edges(int on);
int integral_uses_edges();
int launch_integral(const WeightSet &ws, const double *data, long ncell, int planes, long nx,
                    const int *tr_offsets_dev, int ntransect, double *scratch, double *row, hipStream_t s,
                    int nsteps = 1, long data_stride = 0, long row_stride = 0, const int *rec_cells = nullptr);
// two time steps of the engine's own planes through the (cell, 4 weights) records in ONE gather launch (the record stream is
// read once for both): uvA -> row, uvB -> row + row_stride, where uvX is a step's eU plane followed by its eV plane.
// scratch: 2 * ws.nrec doubles.  The same summation tree per step as launch_integral(planes = 2): the same bits.
// a_interleaved / b_interleaved: that operand is K1's interleaved stream E (FluxArgs::interleaved) instead of two planes; B may
// be interleaved only when A is.
int launch_integral_pair(const Transects &tr, const double *uvA, const double *uvB, long ncell, long nx, double *scratch,
                         double *row, long row_stride, hipStream_t s, bool a_interleaved = false, bool b_interleaved = false);

// What every per-step kernel of a Field reads of one time step (K1's FluxArgs has the same fields, filled from this): the
// fields, the grid, the levels [z0, z1) and the masking / unit settings of uo / vo.
struct StepInput {
    const void *u = nullptr, *v = nullptr;   // base of the time step: (nz, ncell) of the field dtype
    int dtype = NF_F64;
    long ncell = 0, ny = 0, nx = 0;
    int z0 = 0, z1 = 0;
    const double *thickness = nullptr, *arcE = nullptr, *arcN = nullptr;   // device
    double fill = __builtin_nan(""), fill2 = __builtin_nan("");   // NaN = none
    double scale = 1.0;       // 1 or 6371000/1e6
    int sverdrup = 0;
};

// Depth-resolved rows (nf_field_compute_profile): the per-level form of the record path of K3, reading the raw fields of
// one time step.  prof: (nz, row_length) doubles; the kernels write rows [z0, z1) only.  Levels are processed
// kProfileChunk at a time: scratch holds the run sums of one chunk, ws.nrec * kProfileChunk doubles.
// With a carried tracer (t.tau != nullptr; nf_field_compute_tracer_profile) every term is multiplied by tr_face of the tracer at
// its own face, as one level of the tracer transport: 4 + 5 gathers per level, kTracerProfileChunk levels at a time (float64)
// or kTracerProfileChunkF32 (float32: half the registers per gathered value): tracer_profile_chunk(dtype), measured.
// Per-cell layer thicknesses (nf_field_set_cell_thickness): e3u at the index of uo (the east face of the cell), e3v at the
// index of vo, both (nz, ncell) of the field dtype at the base of the step that is read.  e3u == nullptr: the per-level
// thickness of StepInput.  A thickness that is NaN or one of the two markers (compared in the field dtype) counts as 0.
struct CellThick {
    const void *e3u = nullptr, *e3v = nullptr;
    double fill = __builtin_nan(""), fill2 = __builtin_nan("");   // NaN = none
};
// the same for a kernel of dtype T; thick_fixed is fixth() of the definition
template <typename T>
struct ThickIn {
    const T *e3u, *e3v;
    T m1, m2;
};
template <typename T>
inline ThickIn<T> thick_in(const CellThick &c) { return ThickIn<T>{(const T *)c.e3u, (const T *)c.e3v, (T)c.fill, (T)c.fill2}; }
template <typename T>
__device__ inline double thick_fixed(T x, T m1, T m2)
{
    return (x != x || x == m1 || x == m2) ? 0.0 : (double)x;
}

// A tracer at T-points as the kernels of a Field read one time step of it (nf_field_set_tracer*, nf_field_set_class_tracer*):
// the tracer transport, the carried forms of the profiles, the class field and the two axes of the joint classes.
struct TracerIn {
    const void *tau = nullptr;   // base of the time step: (nz, ncell) of the field dtype
    double fill = __builtin_nan(""), fill2 = __builtin_nan("");   // the tracer's own _FillValue / missing_value; NaN = none
    double ref = 0.0;            // reference value subtracted from every face value
    int wrap_x = 1;              // 1: the east face of column nx-1 takes column 0 as its neighbour
};

constexpr int kProfileChunk = 8;
// the volume profile with cell thicknesses: 4 + 4 gathers per level.  Four levels, the 32 gathers per lane that the scalar form
// has in flight: 95 (float64) / 64 (float32) VGPRs, 5 / 8 waves per SIMD, no scratch (the scalar form: 93 / 66, 5 / 7); eight
// levels take 159 / 98 VGPRs and 3 / 4 waves (-Rpass-analysis=kernel-resource-usage)
constexpr int kCellThickProfileChunk = 4;
constexpr int kTracerProfileChunk = 4;
constexpr int kTracerProfileChunkF32 = 8;
inline int tracer_profile_chunk(int dtype) { return dtype == NF_F32 ? kTracerProfileChunkF32 : kTracerProfileChunk; }
struct ProfileArgs {
    StepInput in;
    Transects tr;
    double *scratch = nullptr;
    size_t scratch_len = 0;
    double *prof = nullptr;
    TracerIn t;                  // the carried tracer; t.tau == nullptr: volume rows
    CellThick th;                // volume rows only (t.tau == nullptr): every slot's term takes the thickness at its own face
};
int launch_profile(const ProfileArgs &a, hipStream_t s);

// Section area and area-weighted tracer per level (nf_field_compute_area_profile; DESIGN.md section 4, "Throughflow,
// overturning and gyre parts"): rows (2, nz, row_length) = A, T; the kernels write rows [z0, z1) of both.  The carried tracer is
// required; th.e3u set: every slot's term takes the thickness at its own face.  Levels go area_chunk(dtype) at a time (measured;
// the "area_chunk" knob picks the other candidate): scratch holds 2 * chunk * ws.nrec run sums.
constexpr int kAreaChunk = 4;
constexpr int kAreaChunkF32 = 8;
inline int area_chunk(int dtype) { return dtype == NF_F32 ? kAreaChunkF32 : kAreaChunk; }
int area_chunk_set(int levels);     // 0 = area_chunk(dtype); 2 or 4 (float64), 4 or 8 (float32)
int area_chunk_now(int dtype);
struct AreaArgs {
    StepInput in;                // scale and sverdrup are not read
    Transects tr;
    double *scratch = nullptr;
    size_t scratch_len = 0;
    double *rows = nullptr;
    long nz = 0;
    TracerIn t;                  // the carried tracer
    CellThick th;
};
int launch_area_profile(const AreaArgs &a, hipStream_t s);

// Gross transports per level (nf_field_compute_gross_profile; DESIGN.md section 4, "Gross transports"): rows
// (2, nz, row_length) = P, N, the terms of the profile row split by the direction of the water at their own slot; the kernels
// write rows [z0, z1) of both.  tau set: the carried form (the terms of the tracer profile, split by the sign of the volume
// term); th.e3u set: every slot's term takes the thickness at its own face -- the two combine.  Levels go
// gross_chunk(dtype, carried, cell) at a time (the "gross_chunk" knob picks another candidate): scratch holds
// 2 * chunk * ws.nrec run sums.  Measured (profiles/gross_timing.txt): float32 is fastest with 8 levels in all four forms;
// float64 with 8 in the plain volume form only and with 4 wherever more than four gathers per level are in flight.  Every
// candidate is free of scratch (-Rpass-analysis=kernel-resource-usage; DESIGN.md has the registers).
constexpr int kGrossChunk = 8;
constexpr int kGrossChunkWideF64 = 4;
inline int gross_chunk(int dtype, bool carried, bool cell)
{
    return dtype == NF_F64 && (carried || cell) ? kGrossChunkWideF64 : kGrossChunk;
}
int gross_chunk_set(int levels);    // 0 = gross_chunk(dtype, carried, cell); 2, 4 or 8 (float64), 4 or 8 (float32)
int gross_chunk_now(int dtype, bool carried, bool cell);
struct GrossArgs {
    StepInput in;
    Transects tr;
    double *scratch = nullptr;
    size_t scratch_len = 0;
    double *rows = nullptr;
    long nz = 0;
    TracerIn t;                  // the carried tracer; t.tau == nullptr: volume form
    CellThick th;
};
int launch_gross_profile(const GrossArgs &a, hipStream_t s);

// Crossings (nf_field_compute_crossings; DESIGN.md section 4, "Crossings"): the per-record, per-level values that the profile
// kernels fold away, stored without any scan.  out: (planes, nz, ws.nrec) doubles, out[(p * nz + z) * nrec + k]; the kernel
// writes levels [z0, z1) of every plane.  Volume form (t.tau == nullptr): planes q, g = the terms of the flux profile and the
// section area |w| * (th * arc) of the slots whose velocity is present (no tracer condition).  Carried form: planes q, c, a, b =
// the terms of the flux profile, of the tracer profile, and the two of the area profile.  th.e3u set: every slot's term takes the
// thickness at its own face, in both forms.  Levels go crossing_chunk(dtype, carried, cell) at a time.  Measured
// (profiles/crossings_timing.txt): float32 is fastest with 8 levels in all four forms, float64 with 8 in the plain volume form
// only and with 4 wherever more than four gathers per level are in flight -- the gross profile's rule.  The "crossing_chunk"
// knob picks another candidate; there is no cross-lane arithmetic, so every candidate gives the same bits).  No scratch.
constexpr int kCrossingChunk = 8;
constexpr int kCrossingChunkWideF64 = 4;
inline int crossing_chunk(int dtype, bool carried, bool cell)
{
    return dtype == NF_F64 && (carried || cell) ? kCrossingChunkWideF64 : kCrossingChunk;
}
int crossing_chunk_set(int levels);   // 0 = crossing_chunk(dtype, carried, cell); 2, 4 or 8
int crossing_chunk_now(int dtype, bool carried, bool cell);
struct CrossingArgs {
    StepInput in;
    const WeightSet *ws = nullptr;
    double *out = nullptr;
    long nz = 0;
    TracerIn t;                  // the carried tracer; t.tau == nullptr: volume form
    CellThick th;
};
int launch_crossing_terms(const CrossingArgs &a, hipStream_t s);

// Tracer transport (nf_field_compute_tracer_flux, nf_tracer.hip): K1's vertical integral with every level's velocity
// multiplied by the tracer interpolated to the face, tf = 0.5 (a + b) - ref (DESIGN.md section 4 has the face rule).  Writes
// the two signed planes [eU_tau | eV_tau] of one time step, nothing else; K3 (planes = 2) reduces them.
struct TracerArgs {
    StepInput in;
    TracerIn t;
    double *planes = nullptr; // [2][ncell]: eU_tau, eV_tau
    CellThick th;             // e3u set: fma(fixth(e3u), fixed(u) * tfE, accU), two more aligned streams
};
int launch_tracer_flux(const TracerArgs &a, hipStream_t s);

// The volume step with cell thicknesses (nf_cellthick.hip): K1's vertical integral with the thickness read at the face,
//   accU = fma(fixth(e3u[z, c]), fixed(uo[z, c]), accU), accV likewise with e3v and vo, z ascending over [z0, z1),
// then K1's edge terms.  Writes the two signed planes [eU | eV] at `planes` and raises the running max, as the signed-only
// form of K1 does; launch_expand_planes derives the other four.  in.thickness is not read.
struct CellThickArgs {
    StepInput in;
    CellThick th;
    double *planes = nullptr;             // [2][ncell]: eU, eV
    unsigned long long *maxbits = nullptr;
};
int launch_cellthick_flux(const CellThickArgs &a, hipStream_t s);

// K1's masking of uo / vo outside K1 (profile, class and tracer kernels): NaN or one of the two markers -> 0.  `two`: the second
// marker counts (uv_two_markers: a number that differs from the first; NaN never compares equal, so a kernel without the flag
// passes true).  K1 keeps its own fixed / fixed2: nf_flux.hip is fingerprinted by the benchmark and stays byte for byte.
template <typename T>
inline bool uv_two_markers(T fill, T fill2) { return fill2 == fill2 && !(fill2 == fill); }
template <typename T>
__device__ inline double uv_fixed(T x, T fill, T fill2, bool two = true)
{
    return (x != x || x == fill || (two && x == fill2)) ? 0.0 : (double)x;
}

// The tracer face rule, shared by the tracer transport and the class transport.  A value is present
// when it is not NaN and not one of the tracer's two markers (compared in its dtype).  The raw face value of (a, b), b the
// second cell of the face (has_b = false: the face has none): 0.5 (a + b) in double when both are present, the present one
// when one is; tr_face_raw returns false when neither is (*s is then not a value).
template <typename T>
__device__ inline bool tr_present(T x, T m1, T m2)
{
    return !(x != x || x == m1 || x == m2);
}
template <typename T>
__device__ inline bool tr_face_raw(T a, T b, bool has_b, T m1, T m2, double *s)
{
    const bool pa = tr_present(a, m1, m2), pb = has_b && tr_present(b, m1, m2);
    *s = (pa && pb) ? 0.5 * ((double)a + (double)b) : (pa ? (double)a : (double)b);
    return pa || pb;
}
// the face value of the tracer transport: the raw value minus the reference, 0 without a value
template <typename T>
__device__ inline double tr_face(T a, T b, bool has_b, T m1, T m2, double ref)
{
    double s;
    return tr_face_raw(a, b, has_b, m1, m2, &s) ? s - ref : 0.0;
}

// Volume transport in tracer classes (nf_field_compute_class_transport, nf_integral.hip): rows 0 .. nedges+1 of one time
// step -- row 0: class value x < e[0]; row k: e[k-1] <= x < e[k]; row nedges: x >= e[nedges-1]; row nedges+1: no value
// (tracer missing on both sides of the face, or NaN from +inf beside -inf).  The class value of a face is tr_face_raw of
// the tracer (no reference).  Each per-level term of the profile kernel goes to the row of its own face; the rows are
// built `window` at a time: scratch holds ws.nrec * window run sums.
constexpr int kMaxClassEdges = 1025;
constexpr int kClassWindowMax = 32;
struct ClassArgs {
    StepInput in;
    TracerIn cls;                // the class field; its wrap_x is the rule of every face, its ref is not read
    const double *edges = nullptr;   // device, nedges
    int nedges = 0;
    int window = 0;              // rows per pass over the fields, 1 .. kClassWindowMax
    Transects tr;
    double *scratch = nullptr;
    size_t scratch_len = 0;
    double *rows = nullptr;      // (nedges + 2, row_length)
    // tracer transport in classes (nf_field_compute_class_tracer_transport): every term times tr_face of the carried tracer
    // at its own face.  carry.tau == nullptr: volume transport.  The carried tracer may be the class field itself (the same
    // array with the same markers: one set of gathers) or another array; its wrap_x is not read.
    TracerIn carry;
    // launch_class_remap only: the levels of the arrays -- the class field's levels z0 - 1 and z1 are read where the array has them
    int remap_nz = 0;
};
int launch_class_transport(const ClassArgs &a, hipStream_t s);
// Conservative remapping of the class transport (nf_field_compute_class_remap, nf_integral.hip): the same rows from the same
// terms, each spread over the classes between the class field's values at the layer's two interfaces (k_class_remap_segscan)
int launch_class_remap(const ClassArgs &a, hipStream_t s);

// Transports in true-depth bins (nf_field_compute_depth_transport, nf_integral.hip; the contract is in nemoflux_amd.h): rows
// 0 .. nedges+1 of one time step -- row 0: depth < e[0]; row k: e[k-1] <= depth < e[k]; row nedges: depth >= e[nedges-1];
// row nedges+1: terms of a face whose interface depth is not finite.  Each per-level term of the profile kernel is spread
// uniformly in depth over [D_z, D_z+1], the running sum from `top` of the thicknesses of its own face over ALL levels of the
// array from level 0 on: th.e3u set: fixth(e3) at the slot's face (level_th), read for the levels [0, in.z1) of the step; else
// in.thickness[z].  Terms come from the owned levels [in.z0, in.z1) only.  t.tau set: the carried form (the terms of the tracer
// profile); the two combine.  The rows are built `window` at a time: scratch holds ws.nrec * window run sums.
struct DepthArgs {
    StepInput in;
    const double *edges = nullptr;   // device, nedges
    int nedges = 0;
    double top = 0.0;            // D_0, the depth of the upper interface of level 0
    int window = 0;              // rows per pass over the fields, 1 .. kClassWindowMax
    Transects tr;
    double *scratch = nullptr;
    size_t scratch_len = 0;
    double *rows = nullptr;      // (nedges + 2, row_length)
    TracerIn t;                  // the carried tracer; t.tau == nullptr: volume form
    CellThick th;
};
int launch_depth_transport(const DepthArgs &a, hipStream_t s);

// Transports between surfaces (nf_field_compute_surface_transport, nf_integral.hip; the contract is in nemoflux_amd.h): the
// depth bins with the edges of every face taken from m 2-D fields at T-points -- rows 0 .. m + 1 of one time step, row 0 above
// surface 1, row k between surfaces k and k + 1, row m below surface m, row m + 1 the terms of a face without an edge set or
// with an interface depth that is not finite.  Terms, interface depths, spreading and the window loop are DepthArgs'.
constexpr int kMaxSurfaces = 8;
struct SurfaceSet {
    const void *p[kMaxSurfaces] = {};   // device: step t' of every surface, (ncell) of the field dtype
    int m = 0;
    double fill = __builtin_nan(""), fill2 = __builtin_nan("");   // the surfaces' own markers; NaN = none
    int wrap_x = 1;              // 1: the east face of column nx-1 takes column 0 as its neighbour
};
struct SurfaceArgs {
    StepInput in;
    SurfaceSet sf;
    double top = 0.0;            // D_0, the origin of the surfaces' depths too
    int window = 0;              // rows per pass over the fields, 1 .. kClassWindowMax
    Transects tr;
    double *scratch = nullptr;
    size_t scratch_len = 0;
    double *rows = nullptr;      // (m + 2, row_length)
    TracerIn t;                  // the carried tracer; t.tau == nullptr: volume form
    CellThick th;
};
int launch_surface_transport(const SurfaceArgs &a, hipStream_t s);

// Transport in JOINT classes of two tracers (nf_field_compute_joint_class_transport, nf_integral.hip): axis A is the tracer
// (edges ea, na), axis B the class tracer (edges eb, nb); joint row ra * (nb + 2) + rb, ra / rb the 1-D rows of the face's
// raw value of A / B.  Stage 1 gathers once and writes, per (record, owned level), the four weighted slot terms and their
// four joint rows to the term table; stage 2 bins the table `window` rows at a time.  The table, per owned level zi:
//   terms + (zi * 2 + 0) * nrec: dvec2 (south, east) per record;  terms + (zi * 2 + 1) * nrec: dvec2 (north, west);
//   rows + zi * nrec: 4 x uint16 per record (south, east, north, west; kJointNoRow: the slot contributes nothing)
// -- 40 bytes per (record, level), a wave's loads 64 consecutive 16- or 8-byte elements.  flags: one bit per (block of
// kBlock records, window), words_per_block 32-bit words a block; a clear bit: no term of the block has a row in the window.
constexpr int kMaxJointRows = 16384;
constexpr unsigned kJointNoRow = 0xFFFFu;
constexpr size_t kJointEntryBytes = 40;
struct JointArgs {
    StepInput in;
    TracerIn ta, tb;             // A (its ref: the carried form; its wrap_x: the rule of every face) and B (markers only)
    int carry = 0;               // 1: every term times tr_face of A at its own face
    const double *edges = nullptr;   // device: ea (na doubles) followed by eb (nb doubles)
    int na = 0, nb = 0;
    int window = 0;              // rows per pass over the table, 1 .. kClassWindowMax
    int skip = 1;                // 1: a stage-2 block whose flag is clear does not read the table
    Transects tr;
    char *table = nullptr;       // kJointEntryBytes * nrec * (z1 - z0) bytes
    size_t table_len = 0;
    unsigned *flags = nullptr;   // blocks * words_per_block words
    size_t flags_len = 0;
    double *scratch = nullptr;   // nrec * window run sums
    size_t scratch_len = 0;
    double *rows = nullptr;      // ((na + 2) * (nb + 2), row_length)
};
inline int joint_flag_words(int nrows, int window) { return ((nrows + window - 1) / window + 31) / 32; }
int launch_joint_class_transport(const JointArgs &a, hipStream_t s);

// Gross (inflow / outflow) transports in tracer classes (nf_field_compute_gross_class_transport, nf_integral.hip): the terms of
// the gross profile -- volume form, or carried form with carry.tau set -- sent to the class row of their own face instead of
// their level: rows (2, nedges + 2, row_length) = P, N, row part * (nedges + 2) + r of JointArgs' term table and window bitmap
// (layout above), binned by the joint classes' stage 2.  th.e3u set: every slot's term takes the thickness at its own face.
// Stage 1 issues the gathers of kGrossClassLevels levels together, the joint classes' batch: no instantiation uses scratch
// memory (-Rpass-analysis=kernel-resource-usage; DESIGN.md has the registers and what two levels gave for the widest form).
constexpr int kGrossClassLevels = 4;
struct GrossClassArgs {
    StepInput in;
    TracerIn cls;                // the class field; its wrap_x is the rule of every face, its ref is not read
    TracerIn carry;              // the carried tracer (the class field itself, or another array); tau == nullptr: volume form
    CellThick th;
    const double *edges = nullptr;   // device, nedges
    int nedges = 0;
    int window = 0;              // rows per pass over the table, 1 .. kClassWindowMax
    int skip = 1;                // 1: a stage-2 block whose flag is clear does not read the table
    Transects tr;
    char *table = nullptr;       // kJointEntryBytes * nrec * (z1 - z0) bytes
    size_t table_len = 0;
    unsigned *flags = nullptr;   // blocks * joint_flag_words(2 * (nedges + 2), window) words
    size_t flags_len = 0;
    double *scratch = nullptr;   // nrec * window run sums
    size_t scratch_len = 0;
    double *rows = nullptr;      // (2 * (nedges + 2), row_length)
};
int launch_gross_class_transport(const GrossClassArgs &a, hipStream_t s);

// Remapped gross class transports (nf_field_compute_gross_class_remap, nf_integral.hip; the contract is in nemoflux_amd.h): the
// terms and parts of GrossClassArgs -- rows (2, nedges + 2, row_length) = P, N -- each term spread over the class rows by the
// rule of launch_class_remap instead of going whole to the row of its face (k_gross_remap_segscan).  No term table: like the
// remap it walks the fields once per window of rows, here once per part and window, with ClassArgs' scratch of ws.nrec * window
// run sums.  nz: the levels of the arrays -- the class field's levels z0 - 1 and z1 are read where the array has them; the cell
// thickness is read at the owned levels only.
struct GrossRemapArgs {
    StepInput in;
    TracerIn cls;                // the class field; its wrap_x is the rule of every face, its ref is not read
    TracerIn carry;              // the carried tracer (the class field itself, or another array); tau == nullptr: volume form
    CellThick th;
    const double *edges = nullptr;   // device, nedges
    int nedges = 0;
    int window = 0;              // rows per pass over the fields, 1 .. kClassWindowMax
    Transects tr;
    double *scratch = nullptr;   // nrec * window run sums
    size_t scratch_len = 0;
    double *rows = nullptr;      // (2 * (nedges + 2), row_length)
    int nz = 0;
};
int launch_gross_class_remap(const GrossRemapArgs &a, hipStream_t s);

// Section area and area-weighted tracer in tracer classes (nf_field_compute_class_area, nf_integral.hip): the alpha and beta of
// the area profile sent to the class row of their own face instead of their level: rows (2, nedges + 2, row_length) = A, B, row
// part * (nedges + 2) + r of JointArgs' window bitmap, binned by the joint classes' stage 2.  A table entry holds one term per
// slot and a (record, level) has two, so the table takes TWO entries per (record, owned level) in JointArgs' layout over
// 2 * (z1 - z0) "levels": entries [0, z1 - z0) the alphas, [z1 - z0, 2 (z1 - z0)) the betas -- 80 bytes per (record, level),
// one round of gathers (DESIGN.md section 4 has the choice).  carry: the tracer of the area profile, required; cls: the class
// field, the same array or another.  th.e3u set: every slot's term takes the thickness at its own face.  scale and sverdrup of
// StepInput are not read.  Stage 1 issues the gathers of kClassAreaLevels levels together, the gross class batch.
constexpr int kClassAreaLevels = kGrossClassLevels;
constexpr size_t kClassAreaEntryBytes = 2 * kJointEntryBytes;
struct ClassAreaArgs {
    StepInput in;
    TracerIn cls;                // the class field; its wrap_x is the rule of every face, its ref is not read
    TracerIn carry;              // the carried tracer (the class field itself, or another array)
    CellThick th;
    const double *edges = nullptr;   // device, nedges
    int nedges = 0;
    int window = 0;              // rows per pass over the table, 1 .. kClassWindowMax
    int skip = 1;                // 1: a stage-2 block whose flag is clear does not read the table
    Transects tr;
    char *table = nullptr;       // kClassAreaEntryBytes * nrec * (z1 - z0) bytes
    size_t table_len = 0;
    unsigned *flags = nullptr;   // blocks * joint_flag_words(2 * (nedges + 2), window) words
    size_t flags_len = 0;
    double *scratch = nullptr;   // nrec * window run sums
    size_t scratch_len = 0;
    double *rows = nullptr;      // (2 * (nedges + 2), row_length)
};
int launch_class_area(const ClassAreaArgs &a, hipStream_t s);

// VectorInterp (field.py:90-95,119-120)
// targets_dev: caller order (n,3); sorted_dev: the same points sorted by y; order_dev: caller index of sorted point q
int launch_find_points(const double *xy, long ncell, long row_length, LocatorBoxes *keep, const double *targets_dev, long npts,
                       double periodX, double tol2, unsigned long long *best_dev, long *cell_dev, double *pcoords_dev,
                       hipStream_t s);
int launch_face_vectors(const double *xy, const long *cell_dev, const double *pcoords_dev, long npts, const double *data,
                        long ncell, int planes, double periodX, double *vectors_dev, hipStream_t s);

// datagen
int launch_datagen_bounds(double *blon, double *blat, long ny, long nx, double xmin, double xmax, double ymin,
                          double ymax, double dlon, double dlat, int lat_uses_dx, hipStream_t s);
void datagen_use_rows(int on);   // 0: always the one-cell-per-lane generator kernel (plain division): the row kernel's reference
int launch_datagen_uv(void *u, void *v, int dtype, long t0, long t1, long nt, long nz, long ny, long nx,
                      double xmin, double xmax, double ymin, double ymax, double zmin, double zmax,
                      int lat_uses_dx, int psi, hipStream_t s);

}  // namespace nf
