/*
 * nemoflux_amd.h -- C ABI of libnemoflux_amd.so, the MI355X (gfx950) transect-flux engine.
 *
 * This is the drop-in boundary for nemoflux's hot path.  Two levels:
 *
 *   Level 1  mnt_grid_* / mnt_polylineintegral_*  -- the entry points nemoflux reaches in the
 *            un-vendored `mint` C library through its ctypes wrapper (python-mint >= 1.24.4,
 *            /root/reference/README.md:12).  Same names, argument order, handle convention
 *            (opaque object passed as T**) and error convention (int return, 0 = OK) as mint's
 *            C API, so nemoflux/horizgrid.py:23-24,30,43 and nemoflux/field.py:45-48,102 run
 *            unchanged on top of nemoflux_amd/mint.py.
 *   Level 2  nf_field_*  -- the Field-shaped engine (nemoflux/field.py:15-234): geometry set-up,
 *            per-time-step vertical integration + edge flux (the bandwidth-bound kernel), batched
 *            transect weights and the per-segment / per-transect reduction, with U/V resident in HBM
 *            and (t,z) slab ownership for multi-GPU runs.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in any signature (streams travel as void*).
 *   - every function returns 0 on success, non-zero on error; nf_last_error() gives the message.
 *   - "host" pointers are ordinary CPU memory owned by the caller; "dev" pointers are HBM addresses
 *     of the current device (e.g. torch.Tensor.data_ptr() or nf_malloc()).
 *   - all entry points are synchronous at return unless the name ends in _async.
 *   - there is NO CPU fallback: every compute entry point fails with NF_ERR_NO_DEVICE when no
 *     gfx950 device is usable.
 *   - threads: the reference drives mint from one thread (fluxviz.py:20-23,351) and so may a client.  What holds beyond
 *     that: the error text is per thread; one OBJECT (a PolylineIntegral, a VectorInterp, a field, an inflater) is used by
 *     one thread at a time; different objects may be driven from different host threads even when they share a Grid_t --
 *     the grid's locator cache is built, walked and released under the grid's own lock; the weight-build scratch is a
 *     process-wide pool under a lock.  Giving a Grid_t new points (mnt_grid_build) while another thread still integrates
 *     with objects made on it is the caller's race, as with mint.  nf_tuning_set is NOT thread-safe (see there).
 */
#ifndef NEMOFLUX_AMD_H
#define NEMOFLUX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NF_OK 0
#define NF_ERR_ARG 1        /* bad argument / shape (the reference raises RuntimeError: field.py:135,154) */
#define NF_ERR_STATE 2      /* call order violated (e.g. computeWeights before setGrid) */
#define NF_ERR_HIP 3        /* a HIP runtime call failed */
#define NF_ERR_NO_DEVICE 4  /* no usable GPU: the engine never falls back to the CPU */
#define NF_ERR_HOST 5       /* host-side failure (out of host memory, file write error); no C++ exception ever
                               crosses this ABI */

#define NF_F64 0
#define NF_F32 1

/* mint.CELL_BY_CELL_DATA / mint.UNIQUE_EDGE_DATA (field.py:102 uses the former) */
#define MNT_CELL_BY_CELL_DATA 0
#define MNT_UNIQUE_EDGE_DATA 1

/* ------------------------------------------------------------------ library / device plumbing */
const char *nf_last_error(void);
int nf_version(void);
int nf_device_count(int *count);
int nf_set_device(int device);
int nf_device_name(char *buf, int buflen); /* e.g. "gfx950:..." */
int nf_malloc(void **dev, size_t bytes);
int nf_free(void *dev);
int nf_host_alloc(void **host, size_t bytes); /* pinned host memory (fast D2H into numpy views) */
int nf_host_free(void *host);
int nf_memcpy_h2d(void *dev, const void *host, size_t bytes);
int nf_memcpy_d2h(void *host, const void *dev, size_t bytes);
int nf_memset(void *dev, int value, size_t bytes);
int nf_synchronize(void);
/* Weight builds and point searches keep their scratch memory between calls while it is small (a process-wide pool of at most
 * 4 idle scratches of at most 1 GiB of HBM each: a viewer makes one PolylineIntegral per transect and each build would
 * otherwise pay a dozen hipMalloc / hipFree pairs).  A build checks a scratch out of the pool and hands it back, whichever
 * host thread runs it, so threads that end leave nothing behind.  This call frees every idle scratch of the process
 * (the Python package calls it at interpreter exit). */
int nf_release_scratch(void);
/* host-side file decoding helper: undo HDF5's shuffle filter (es byte planes of n elements -> n elements) */
int nf_host_unshuffle(const void *src, void *dst, size_t n, int es);
/* host-side file staging helper: copy n byte ranges (addresses as integers) with nthreads native threads -- the compressed
 * chunks of a group of time steps out of the mapped file into a pinned staging buffer (field.py:149 reads them one by one) */
int nf_host_gather(const unsigned long long *src_addr, const unsigned long long *dst_addr, const long long *len, long long n,
                   int nthreads);
/* tuning knobs for A/B measurements inside one process: "flux_variant" (0 = default store form, 5 = the other one; see nf_flux.hip),
 * "xcd_map" (1 = on), "batch_steps" (1 = small grids run all time steps in one launch), "field_split" (-1 = one-step launches
 * of fewer than 20 000 wavefronts integrate uo and vo in different wavefronts, 0 = never, 1 = always), "edge_weights", "datagen_rows"
 * (0 = the generator's one-cell-per-lane kernel with plain division, the reference of its row kernel), "west_shift" (0 = the
 * west slots of integratedVelocity as 8-byte stores, the form before round 5), "batch_cellsteps_m" (all-steps-in-one-launch
 * limit in Mi cell-steps, 32), "partial_step_planes" (1 = six-plane epilogue on a rank's partial time steps), "graph" (0 =
 * no graph replay of a pass).  The library reads NO environment variable: these calls are the only switches.
 * NOT thread-safe: the knobs are plain process-wide variables read by every later launch of every thread; set them before the
 * objects they affect are used and from one thread only (the reference drives mint from a single thread; A/B tools
 * and the bench's --knob do the same).  A product run never needs to call this. */
int nf_tuning_set(const char *name, int value);

/* ------------------------------------------------------------------ Level 1: mint-shaped API */
typedef struct Grid_t Grid_t;
typedef struct PolylineIntegral_t PolylineIntegral_t;

/* mint.Grid()                                   horizgrid.py:23 */
int mnt_grid_new(Grid_t **self);
int mnt_grid_del(Grid_t **self);
/* mint.Grid.setPoints(points (ncell,4,3) float64)  horizgrid.py:24.  `points` is BORROWED (host) and
 * must outlive the grid, as in mint; the corner (lon,lat) pairs are uploaded to HBM by mnt_grid_build. */
int mnt_grid_setPointsPtr(Grid_t **self, double *points);
int mnt_grid_build(Grid_t **self, int nVertsPerCell, long long ncells);
/* extension (not in mint): the cells handed to setPoints are the rows of a (ny, nx) grid, nx = rowLength -- what
 * horizgrid.py:17-22 flattens.  Only a hint: the weights do not depend on it, the locator groups the cells in 4 x 4 blocks
 * instead of 16 consecutive ones and long target lines are located several times faster.  0 = unknown (default). */
int mnt_grid_setRowLength(Grid_t **self, long long rowLength);
/* mint.Grid.getNumberOfCells()                  horizgrid.py:30 */
int mnt_grid_getNumberOfCells(Grid_t **self, size_t *numCells);
/* mint.Grid.dump(fileName): legacy-VTK unstructured grid  horizgrid.py:43 */
int mnt_grid_dump(Grid_t **self, const char *fileName);

/* mint.PolylineIntegral()                       field.py:45 */
int mnt_polylineintegral_new(PolylineIntegral_t **self);
int mnt_polylineintegral_del(PolylineIntegral_t **self);
/* .setGrid(grid)                                field.py:46 */
int mnt_polylineintegral_setGrid(PolylineIntegral_t **self, Grid_t *grid);
/* .buildLocator(numCellsPerBucket=128, periodX=360., enableFolding=False)   field.py:47
 * The locator is a 16-fold hierarchy of bounding boxes over the cells, built at the first computeWeights / findPoints on the
 * grid and kept by the grid (nf_locator.h); numCellsPerBucket must be positive and has nothing to tune; enableFolding != 0
 * is rejected (nemoflux never enables it).  periodX > 0: target lines are also tried one period to the west and to the east,
 * and every cell's corners are brought to within periodX/2 of its corner 0 before the cell is used (a global file stores
 * bounds_lon wrapped into one period, so the cells on the cut have corners ~355 degrees apart: datagen.py:161-166 is the
 * reference's own form of this rule); the grid's points themselves are not touched. */
int mnt_polylineintegral_buildLocator(PolylineIntegral_t **self, int numCellsPerBucket, double periodX,
                                      int enableFolding);
/* .computeWeights(xyz (npoints,3), counterclock=False)   field.py:48
 * A cell the weights are not defined on -- a quad that is not convex in the (lon,lat) plane, one with a corner AT a
 * geographic pole (the cells around the pole of a rotated grid) or one that CONTAINS a pole -- that a target segment
 * overlaps over a positive length is left out (policy 'skip', the default of this mint-shaped level since round 6: mint's
 * computeWeights has no error path there, field.py:44-49): the rest of the line is integrated,
 * mnt_polylineintegral_getCoverage reports < 1 for the segment and mnt_polylineintegral_getNumberOfDroppedCrossings says
 * how many such crossings were left out -- never a silent number.  With mnt_polylineintegral_setUnsupportedCells(0) the
 * call returns NF_ERR_ARG (with the cell id in nf_last_error) instead.  NF_ERR_ARG naming
 * the segment, too, when some stretch of a target segment lies in two cells that do not hold the same sub-segment (coverage
 * > 1 + 1e-8 AND the excess, as a length, > 1e-9 max(1, |coordinates|) degrees: overlapping cells, e.g. a date-line-wrapped
 * grid with periodX = 0): that stretch would be counted twice.  (The length condition keeps rounding noise on target
 * segments of ~1e-8 degrees and shorter -- near-duplicate vertices on a grid node -- from refusing a whole line.)
 * mnt_polylineintegral_getCoverage still answers after that error.  Cells with a corner that is not a finite number take
 * part in nothing. */
int mnt_polylineintegral_computeWeights(PolylineIntegral_t **self, int npoints, const double xyz[],
                                        int counterclock);
/* extension (not in mint): what computeWeights does with such a cell.  skip = 1 (default): the cell contributes nothing --
 * the rest of the line is integrated and mnt_polylineintegral_getCoverage reports the fraction of every target segment
 * that was (real ORCA grids with a few distorted polar cells far from the transect's physics; mint itself returns a number
 * there, pinned by nothing in the reference).  skip = 0: NF_ERR_ARG naming the cell. */
int mnt_polylineintegral_setUnsupportedCells(PolylineIntegral_t **self, int skip);
/* extension: (cell, target-segment image) crossings of unsupported cells the last computeWeights left out (0 unless the
 * policy is 'skip' and the line meets such cells) */
int mnt_polylineintegral_getNumberOfDroppedCrossings(PolylineIntegral_t **self, size_t *n);
/* extension (not in mint): what computeWeights does with a target segment that is covered more than once (see above).
 * warn = 0 (default): NF_ERR_ARG.  warn = 1: the weights are built as mint would build them -- the stretch counts twice --
 * and mnt_polylineintegral_getCoverage reports > 1 for the segment (the Python wrapper warns). */
int mnt_polylineintegral_setOverlappingCells(PolylineIntegral_t **self, int warn);
/* .getIntegral(data (ncell,4) float64 HOST, placement) -> *result   field.py:102, fluxplot.py:56
 * Host data is staged SPARSELY: only the 32 bytes of every cell the weights touch are gathered (pinned buffer) and sent
 * to HBM -- the cost follows the number of weights, not the size of the grid, like mint's own sparse dot -- and the same
 * kernels run on them: the result has the bits of ...getIntegralDev on the whole array (see that for resident data). */
int mnt_polylineintegral_getIntegral(PolylineIntegral_t **self, const double data[], int placement,
                                     double *result);
/* extensions (not in mint): device-resident data, per-target-segment sums, weight read-back */
int mnt_polylineintegral_getIntegralDev(PolylineIntegral_t **self, const double *data_dev, int placement,
                                        double *result, double *seg_totals_host /* nseg or NULL */);
/* coverage[s] = fraction of target segment s that lies inside cells of the grid (1 = inside, counted once; < 1 = part of it
 * lies in no cell and contributes nothing; > 1 is refused by computeWeights); see nf_field_get_coverage.  npoints-1 values. */
int mnt_polylineintegral_getCoverage(PolylineIntegral_t **self, double *coverage);
int mnt_polylineintegral_getNumberOfWeights(PolylineIntegral_t **self, size_t *n);
int mnt_polylineintegral_getWeights(PolylineIntegral_t **self, int64_t *cell_edge, double *weight, int *seg);

/* mint.VectorInterp: the arrows on the target line                field.py:90-95, 119-120 */
typedef struct VectorInterp_t VectorInterp_t;
int mnt_vectorinterp_new(VectorInterp_t **self);
int mnt_vectorinterp_del(VectorInterp_t **self);
/* .setGrid(grid)                                field.py:91 */
int mnt_vectorinterp_setGrid(VectorInterp_t **self, Grid_t *grid);
/* .buildLocator(numCellsPerBucket=128, periodX=360.)   field.py:92 */
int mnt_vectorinterp_buildLocator(VectorInterp_t **self, int numCellsPerBucket, double periodX, int enableFolding);
/* .findPoints(targetPoints (n,3) host, tol2=1.e-12)    field.py:93; *numNotFound (may be NULL) counts points outside */
int mnt_vectorinterp_findPoints(VectorInterp_t **self, size_t numPoints, const double targetPoints[], double tol2,
                                size_t *numNotFound);
/* .getFaceVectors(data (ncell,4) host, placement=0) -> vectors (n,3) host   field.py:94-95,119
 * Only the rows of the located cells travel to HBM (n x 32 B); same bits as ...getFaceVectorsDev on the whole array. */
int mnt_vectorinterp_getFaceVectors(VectorInterp_t **self, const double data[], int placement, double vectors[]);
/* extensions: data resident in HBM (layout 0 = (ncell,4), 1 = the engine's [4][ncell] planes); located cells */
int mnt_vectorinterp_getFaceVectorsDev(VectorInterp_t **self, const double *data_dev, int layout, double vectors[]);
int mnt_vectorinterp_getCells(VectorInterp_t **self, long long *cell_ids, double *pcoords /* (n,2) */);

/* ------------------------------------------------------------------ Level 2: Field-shaped engine */
typedef struct nf_field nf_field;

int nf_field_new(nf_field **self);
int nf_field_del(nf_field **self);
/* HIP stream all of this field's kernels and copies are issued on (NULL = the null stream, which is
 * also torch's default current stream). */
int nf_field_set_stream(nf_field **self, void *hip_stream);
/* Cell bounds (field.py:22-24, horizgrid.py:12-24): bounds_lon/lat (ny,nx,4), dtype NF_F64 (datagen) or
 * NF_F32 (real NEMO), host (on_device=0) or HBM (1).  Runs the geometry kernel: corner table, great-circle
 * edge lengths (field.py:170-181), lon/lat box (field.py:27-30). */
int nf_field_set_bounds(nf_field **self, const void *bounds_lon, const void *bounds_lat, long ny, long nx,
                        int dtype, int on_device);
/* Layer thickness = deptht_bounds[:,1]-deptht_bounds[:,0] (field.py:51), host, nz values. */
int nf_field_set_thickness(nf_field **self, const double *thickness, long nz);
/* uo/vo (nt,nz,ny,nx) x-fastest (field.py:34-35,122-136).  on_device=1: HBM pointers, used in place (no
 * copy).  on_device=0: host arrays, one time step is staged through HBM per compute call.  fill_value:
 * the variable's _FillValue (datagen.py:191,204: 1e20) -- NaN and fill_value both count as missing ->
 * 0 (field.py:157); pass NaN for "no _FillValue". */
int nf_field_set_uv(nf_field **self, const void *u, const void *v, long nt, int dtype, int on_device,
                    double fill_value);
/* A second value that counts as missing -> 0: the CF attribute missing_value when it differs from _FillValue (xarray's
 * decode_cf, which the reference relies on at field.py:34-35, masks both).  Compared in the fields' dtype; NaN = none. */
int nf_field_set_missing_value(nf_field **self, double missing_value);
/* field.py:19,225-228: scale fluxes by 6371000/1e6 */
int nf_field_set_sverdrup(nf_field **self, int sverdrup);
/* Compact resident mode (default off).  The reference stores, per time step, the (ncell,4) array whose slots 0 and 3
 * are copies of the neighbours' slots 2 and 1 (field.py:209-223) and the two |.| arrays (field.py:231-232).  With
 * compact != 0 the flux kernel keeps only the two signed arrays (eU, eV) resident -- all the transect reduction reads --
 * and the other four are derived, bit-identically, when nf_field_read_step / nf_field_device_ptr ask for them:
 * 104 instead of 311 MB of stores per step on the ORCA12-like grid.  Batch drivers (fluxplot.py:51-59) never ask. */
int nf_field_set_compact(nf_field **self, int compact);

/* Multi-GPU ownership: this rank integrates the flattened slabs s = t*nz + z in [s_begin, s_end)
 * (SURVEY.md section 8e).  Default: all of them. */
int nf_field_set_slab_range(nf_field **self, long s_begin, long s_end);
/* Transects (field.py:43-49): add polylines, then build all weights in one batched pass.
 * xyz: (npts,3) host.  *transect_id receives the index. */
int nf_field_add_transect(nf_field **self, const double *xyz, int npts, int counterclock, int *transect_id);
/* same policy switch as mnt_polylineintegral_setUnsupportedCells, for the batched build below; call before build_weights.
 * The default of THIS level is 0 (refuse): a batch driver should hear about a transect it cannot integrate in full. */
int nf_field_set_unsupported_cells(nf_field **self, int skip);
/* crossings of unsupported cells the last nf_field_build_weights left out (policy 'skip'), over all transects */
int nf_field_num_dropped_crossings(nf_field **self, size_t *n);
/* same policy switch as mnt_polylineintegral_setOverlappingCells, for the batched build below; call before build_weights */
int nf_field_set_overlapping_cells(nf_field **self, int warn);
int nf_field_build_weights(nf_field **self, int numCellsPerBucket, double periodX);
int nf_field_num_transects(nf_field **self, int *n);
int nf_field_num_segments(nf_field **self, int *nseg_total);             /* over all transects */
int nf_field_segment_offsets(nf_field **self, int *offsets /* ntransect+1 */);
int nf_field_num_weights(nf_field **self, size_t *n);
int nf_field_get_weights(nf_field **self, int64_t *cell_edge, double *weight, int *seg_global);
/* The same weights as the engine's own reduction uses them: folded onto the unique edges of the resident signed planes.
 * The south / west slots of integratedVelocity are copies of the neighbours' north / east values (field.py:219-223, row 0's
 * south slot is never written), so each (cell, edge) weight belongs to one element of [eU | eV] (elem in [0, 2*ncell):
 * eU[c] = c, eV[c] = ncell + c) and the weights that meet on an element are summed per target segment.  Sorted by
 * (segment, elem).  mint has no counterpart; nf_field_get_weights above stays the mint-shaped view. */
/* Fraction of every target segment (nseg_total values, transect after transect) that lies inside cells of the grid: 1 =
 * inside, each point counted once; less = part of the segment is outside the grid and contributes nothing (mint warns
 * when its own sum of coefficient * (tb - ta) is not 1 [recall]; here the caller can look). */
int nf_field_get_coverage(nf_field **self, double *coverage);
int nf_field_num_edge_weights(nf_field **self, size_t *n);
int nf_field_get_edge_weights(nf_field **self, int *elem, int *seg_global, double *weight);
/* Length of one output row: nseg_total + ntransect doubles = [per-segment sums | per-transect sums]. */
int nf_field_row_length(nf_field **self, int *n);

/* One time step (Field.update + getFluxText's integrals: field.py:112-120,98-103): vertical integral of
 * this rank's slabs of step tIndex, edge fluxes into the resident integratedVelocity, then the transect
 * reduction.  row_host (row_length doubles) may be NULL. */
int nf_field_compute_flux(nf_field **self, long tIndex, double *row_host);
/* All nt steps back to back, asynchronously on the field's stream; rows_dev: HBM (nt, row_length),
 * fully overwritten (zeros where this rank owns no slab).  This is the timed "step" of bench.py. */
int nf_field_compute_all_async(nf_field **self, double *rows_dev);
/* Depth-resolved rows of time step tIndex: prof (nz, row_length) doubles, level z's row = [segments | transects] of the
 * flux carried by that level alone.  Levels this rank does not own (slab range) get exact zeros, so the RCCL / gloo
 * sum of the ranks' profiles is the full profile.  Leaves the resident planes, |.| arrays, running max and a captured
 * pass untouched. */
int nf_field_compute_profile(nf_field **self, long tIndex, double *prof_host);        /* synchronous, host */
int nf_field_compute_profile_async(nf_field **self, long tIndex, double *prof_dev);   /* HBM, on the field's stream */
/* Tracer transport across the transects (heat, salt): rows [segments | transects] of the integral of u * tau_face over the
 * owned levels.  tau sits at T-points; for cell (j, i) and level z, a = tau[t,z,j,i], the east (U) face's b = tau[t,z,j,i+1]
 * (column nx-1: tau[t,z,j,0] when wrap_x is on, else no b), the north (V) face's b = tau[t,z,j+1,i] (last row: no b).  A
 * value is present when it is not NaN and not one of the tracer's own two markers (compared in its dtype).  Face value, in
 * double: both present 0.5*(a+b) - ref, one present that value - ref, neither 0.  acc = fma(th_z, fixed(u) * tf, acc) over
 * the owned levels, z ascending (fixed = the masking of uo/vo with their markers), eU_tau = +accU * arcE, eV_tau = -accV *
 * arcN, each times the Sverdrup scale when it is on; the transect reduction is the one of the volume rows.  Units: tracer x
 * volume-flux units (watts: times rho0 * c_p, and 1e6 in Sverdrup mode).  tau == ref + 1 gives the volume rows bit for bit.
 * Steps this rank does not touch (slab range) get exact zeros, so the ranks' rows sum to the full ones.  None of these calls
 * changes the resident planes, |.| arrays, running max or a captured pass; the setters do not invalidate a captured pass. */
/* tracer at T-points (nt,nz,ny,nx), same nt/nz/ny/nx and dtype as uo/vo; host (staged per step, owned levels only) or HBM */
int nf_field_set_tracer(nf_field **self, const void *tracer, long nt, int dtype, int on_device, double fill_value);
int nf_field_set_tracer_missing_value(nf_field **self, double missing_value);  /* NaN = none */
int nf_field_set_tracer_reference(nf_field **self, double ref);                /* default 0 */
int nf_field_set_tracer_wrap(nf_field **self, int wrap_x);                     /* default 1 */
int nf_field_compute_tracer_flux(nf_field **self, long tIndex, double *row_host);   /* row_length doubles */
int nf_field_compute_tracer_all_async(nf_field **self, double *rows_dev);           /* (nt, row_length) in HBM */
/* Volume transport in tracer classes (by temperature, salinity or potential density: overturning in density space).  The
 * tracer of nf_field_set_tracer (its markers and wrap_x; NOT its reference) gives every U / V face a class value x: 0.5*(a+b)
 * in double when both cells beside the face have a value, the present one when one has, none when neither has (a and b as
 * in the tracer block above).  With the class edges e[0] < ... < e[nedges-1] one time step gives nedges + 2 rows, each
 * [segments | transects]: row 0 x < e[0]; row k (1 <= k <= nedges-1) e[k-1] <= x < e[k]; row nedges x >= e[nedges-1] (+inf
 * included); row nedges+1 no class value (also NaN: +inf beside -inf).  The flux that is binned is the per-level term of
 * nf_field_compute_profile: each (record, level, slot) term goes to the row of its own face (the west slot is the east face
 * of the west cell, the south slot the north face of the south cell), so the sum of all rows is the volume row up to
 * rounding, and tau = level index with edges -0.5, 0.5, ... gives the profile rows bit for bit.  Summation order is fixed
 * (levels ascending, slots in order, then the transect reduction): no atomics, bitwise reproducible.  Owned levels only;
 * steps this rank does not touch get exact zeros.  None of these calls changes the resident planes, |.| arrays, running max,
 * the tracer rows or a captured pass.  Compute before set_tracer or set_class_edges: NF_ERR_STATE. */
/* 2 <= nedges <= 1025, finite, strictly increasing (else NF_ERR_ARG); host copy, uploaded by the next compute */
int nf_field_set_class_edges(nf_field **self, const double *edges, int nedges);
int nf_field_compute_class_transport(nf_field **self, long tIndex, double *rows_host);        /* (nedges+2, row_length) */
int nf_field_compute_class_transport_async(nf_field **self, long tIndex, double *rows_dev);   /* HBM, field's stream */
/* Transport in JOINT classes of two tracers (theta and S, sigma and theta: the volumetric T-S census of a section; its
 * cumulative sum along one axis is the thermohaline streamfunction).  Axis A is the tracer of nf_field_set_tracer with the
 * edges edges_a, axis B the class tracer of nf_field_set_class_tracer with the edges edges_b; both tracers are required.  A
 * face has the 1-D row ra of A's raw face value among edges_a and rb of B's among edges_b, each as defined above (no value
 * or NaN: na + 1 / nb + 1); its term goes to the joint row ra * (nb + 2) + rb.  One time step gives (na + 2) * (nb + 2) rows
 * of row_length doubles, written whole, exact zeros where nothing falls.  carry = 0: the per-level volume terms of
 * nf_field_compute_class_transport; carry = 1: every term times tf of the tracer A at its own face, reference subtracted, as in
 * nf_field_compute_class_tracer_transport.  The accumulation order and the summation tree are those of the 1-D forms: the rows
 * are bitwise reproducible, do not depend on the tuning knobs "joint_window" (1 .. 32 rows per pass, default 32) and
 * "joint_skip" (0 / 1), and an axis with a single occupied class gives the 1-D rows of the other axis bit for bit.  The fields
 * are gathered once per call into a term table that the handle owns: 40 bytes x records x owned levels of HBM, allocated on
 * first use, dropped with the weights; when it cannot be allocated the call fails with NF_ERR_HIP and names the size.
 * Each edge set: 2 <= n <= 1025, finite, strictly increasing, and (na + 2) * (nb + 2) <= 16384 (else NF_ERR_ARG naming the
 * count); two NULLs clear the edges.  This state is separate from nf_field_set_class_edges: the 1-D forms do not see it.
 * Owned levels only (set_slab_range).  Compute before set_tracer, set_class_tracer or set_joint_class_edges: NF_ERR_STATE;
 * with a cell thickness set: NF_ERR_STATE, as the 1-D class forms.  The calls change nothing else: not the resident planes,
 * the running max, the last row, the tracer planes, the 1-D class rows or a captured pass. */
int nf_field_set_joint_class_edges(nf_field **self, const double *edges_a, int na, const double *edges_b, int nb);
int nf_field_compute_joint_class_transport(nf_field **self, long tIndex, int carry, double *rows_host);
int nf_field_compute_joint_class_transport_async(nf_field **self, long tIndex, int carry, double *rows_dev);   /* HBM */
/* Depth- and class-resolved tracer transports: the two forms above with the tracer of nf_field_set_tracer carried by the flow.
 * Every per-level term fma(th_z, fixed(x), 0) * arc of nf_field_compute_profile becomes fma(th_z, fixed(x) * tf, 0) * arc, tf
 * the face value of the tracer block (markers, reference and wrap_x included) at the slot's own face: east slot = east face
 * of the cell, north slot = its north face, west slot = east face of the west cell, south slot = north face of the south cell.
 * That is one level of the tracer transport's accumulation, so tau == ref + 1 gives the volume forms bit for bit, and level
 * z's row of the tracer profile is the nf_field_compute_tracer_flux row of a field whose only layer with a thickness is z.
 * Tracer profile: prof (nz, row_length), row z = [segments | transects] of the tracer transport of level z alone; levels this
 * rank does not own get exact zeros; the sum over z is the tracer row up to rounding. */
int nf_field_compute_tracer_profile(nf_field **self, long tIndex, double *prof_host);        /* synchronous, host */
int nf_field_compute_tracer_profile_async(nf_field **self, long tIndex, double *prof_dev);   /* HBM, on the field's stream */
/* Section area and area-weighted tracer, level by level: what splits a tracer transport into the part carried by the net flow
 * through the section (throughflow), by the vertical overturning and by horizontal correlations (gyre).  Records, slots,
 * faces and the neighbour rule are those of nf_field_compute_profile and the tracer block: east slot = east face of c, north
 * slot = north face of c, west slot = east face of the west cell (periodic copy in column 0), south slot = north face of the
 * south cell (nothing on row 0).  For step t, level z and a record's slot q with weight w_q, a the cell the face belongs to:
 * the face COUNTS when (1) its velocity -- uo[t,z,a] for east and west slots, vo[t,z,a] for north and south slots -- is
 * present: not NaN and not one of the uo/vo markers (the comparison of fixed()); (2) the face value x of the tracer of
 * nf_field_set_tracer exists (its markers and wrap_x apply) and is finite; (3) the slot is not the south slot of row 0.  Then
 *   area term    alpha = |w_q| * (th_q * arc_q)      (0 when the face does not count)
 *   tracer term  beta  = alpha * (x - ref)
 * arc_q = arcE[a] or arcN[a] (positive); th_q = thickness[z], or with a cell thickness set fixth(e3u[t',z,a]) / fixth(e3v[t',z,a])
 * as in the cell-thickness profile (a thickness of 0 or a marker removes the face); ref the tracer reference.  NO Sverdrup
 * scale: only ratios of these rows are used.  rows (2, nz, row_length): A(z) = sum of alpha, then T(z) = sum of beta, each row
 * [segments | transects], the transect columns the sums of their segments; slots are added south, east, north, west, then the
 * fixed tree of the transect reduction: no atomics, bitwise reproducible.  Levels this rank does not own are exact zeros.  For
 * a line that cuts cells obliquely A is the staircase area (zonal plus meridional extent): a weight for the mean, not a
 * geometric length.  tau == ref + 1 (ref an integer) gives T == A bit for bit; the rows do not depend on the values of uo / vo,
 * only on where they are present.
 * Decomposition (host, float64, AFTER any all-reduce over ranks: it is not linear), per column, with V(z) the rows of
 * nf_field_compute_profile and H the row of nf_field_compute_tracer_flux:
 *   m(z) = T(z) / A(z) (0 where A(z) = 0),  M = sum_z T / sum_z A (0 where the sum is 0)
 *   throughflow = (sum_z V(z)) * M,  overturning = sum_z V(z) * (m(z) - M),  gyre = H - throughflow - overturning.
 * Compute before set_tracer: NF_ERR_STATE.  Host-resident uo / vo, tracer and time-varying cell thickness are staged per
 * step.  The calls change neither the resident planes, |.| arrays, running max, last row, tracer planes nor a captured pass. */
int nf_field_compute_area_profile(nf_field **self, long tIndex, double *rows_host);       /* (2, nz, row_length): A, T */
int nf_field_compute_area_profile_async(nf_field **self, long tIndex, double *rows_dev);  /* HBM, field's stream */
/* Gross transports, level by level: how much goes through the section in the direction nf_field_compute counts positive and
 * how much comes back -- the inflow and the outflow of a strait, a recirculation -- where every other row is their net.
 * Records, slots, faces and the neighbour rule are those of nf_field_compute_profile.  For step t, level z and a record's slot
 * with weight w:
 *   water term    q = w * d,  d the slot's value of the profile: +fma(th, fixed(uo), 0) * arcE for the east and west slots,
 *                 -fma(th, fixed(vo), 0) * arcN for the north and south slots, times 6.371 in Sverdrup mode, 0 for the south slot
 *                 of row 0; th = thickness[z], or with a cell thickness set fixth(e3u) / fixth(e3v) at the slot's own face
 *   carried term  c = q (carry = 0), or the slot's term of the tracer profile (carry = 1): the same with fixed(.) * tf, tf the
 *                 face value of the tracer of nf_field_set_tracer minus its reference, 0 for a face without a value
 *   P(z) = sum of c over the slots with q > 0,   N(z) = sum of c over the slots with q < 0;   q == 0: in neither.
 * The carried form is split by the direction of the WATER, not by the sign of its own term: P is what the flow carries forward,
 * N what it carries back.  P + N is the row of nf_field_compute_profile (carry = 0) or nf_field_compute_tracer_profile
 * (carry = 1) up to rounding; with carry = 0, P >= 0 >= N and P - N is the sum of |terms|.  carry = 1 takes a cell thickness
 * too (the tracer profile does not yet).  rows (2, nz, row_length): P then N, each row [segments | transects].  A lane adds its
 * four slots south, east, north, west into +0.0 for P and for N alike (a slot that belongs to the other part as +0.0), then the
 * fixed tree of the transect reduction follows: no atomics, bitwise reproducible, and an order that does not depend on the
 * signs -- negating uo and vo gives P' == -N and N' == -P bit for bit, tau == ref + 1 gives the carry = 0 rows bit for bit.
 * Levels this rank does not own are exact zeros.  carry other than 0 or 1: NF_ERR_ARG; carry = 1 before set_tracer:
 * NF_ERR_STATE.  Host-resident uo / vo, tracer and time-varying cell thickness are staged per step.  The calls change neither
 * the resident planes, |.| arrays, running max, last row, tracer planes nor a captured pass.  Mean tracer of the inflow:
 * P(carry = 1) / P(carry = 0) + ref, where the tracer is present wherever the velocity is. */
int nf_field_compute_gross_profile(nf_field **self, long tIndex, int carry, double *rows_host);       /* (2, nz, row_length): P, N */
int nf_field_compute_gross_profile_async(nf_field **self, long tIndex, int carry, double *rows_dev);  /* HBM, field's stream */
/* Crossings: the integrand of every other row.  A crossing is one record of the weights: the piece of one target segment inside
 * one grid cell.  nf_field_num_crossings gives their number ncross = nf_field_num_weights / 4; nf_field_get_crossings gives, in
 * record order (by segment, then along the segment), the global segment, the cell and the piece's parameters 0 <= ta < tb <= 1
 * on its own target segment (also for a piece found through a periodic image).  Identical duplicates (halo columns, a north-fold
 * row) keep their separate records with the same [ta, tb] and half the weight each.  Both calls need built weights (after
 * nf_field_add_transect without nf_field_build_weights: NF_ERR_STATE, like the compute calls); nf_field_get_crossings is a
 * blocking readback meant to be called once per weight build.
 * nf_field_compute_crossings gives, for step t, every level z and every crossing k, out[(p * nz + z) * ncross + k]:
 *   carry = 0, planes (q, g):  q = the sum over the record's four slots of w * d, d the slot's value of nf_field_compute_profile
 *                              (see nf_field_compute_gross_profile's water term); g = the sum of |w| * (th * arc) over the slots
 *                              whose velocity is present (not NaN, not a marker), without the south slot of row 0: the section
 *                              area of the piece, no tracer condition
 *   carry = 1, planes (q, c, a, b):  q as above; c = the record's term of nf_field_compute_tracer_profile (every slot's d with
 *                              fixed(.) * tf); a, b = the record's terms of nf_field_compute_area_profile (A and T)
 * th = thickness[z], or with a cell thickness set fixth(e3u) / fixth(e3v) at the slot's own face, in both forms.  q and c take
 * the Sverdrup scale when it is on; g, a and b never do.  The four slots are added south, east, north, west, ((s + e) + n) + w,
 * with the expressions of the profile kernels: the sum of a plane over the records of a target segment is that segment's column
 * of nf_field_compute_profile (q), nf_field_compute_tracer_profile or P + N of nf_field_compute_gross_profile(carry = 1) (c),
 * nf_field_compute_area_profile (a, b) up to the rounding of the sum, and bit for bit where the segment has one record.  There
 * is no reduction at all, so sharded ranks' planes add up exactly.  Levels this rank does not own are exact zeros.  carry other
 * than 0 or 1: NF_ERR_ARG; carry = 1 before set_tracer: NF_ERR_STATE.  Host-resident uo / vo, tracer and time-varying cell
 * thickness are staged per step.  The calls change neither the resident planes, |.| arrays, running max, last row, tracer
 * planes, class / joint rows nor a captured pass. */
int nf_field_num_crossings(nf_field **self, size_t *n);   /* = num_weights / 4 */
int nf_field_get_crossings(nf_field **self, int *seg_global, int64_t *cell, double *ta, double *tb);
int nf_field_compute_crossings(nf_field **self, long tIndex, int carry, double *out_host);       /* (carry ? 4 : 2, nz, ncross) */
int nf_field_compute_crossings_async(nf_field **self, long tIndex, int carry, double *out_dev);  /* HBM, field's stream */
/* Gross transports in tracer classes: the inflow and the outflow of every class -- the dense overflow against the light water
 * above it, the two layers of a strait, a recirculating limb that the net class transport hides.  Needs nf_field_set_tracer
 * and nf_field_set_class_edges (else NF_ERR_STATE, as nf_field_compute_class_transport).  One time step t over the owned
 * levels; for every weight record and every slot i, in the order south, east, north, west:
 *   d_i  the slot's water term of nf_field_compute_gross_profile: the masked velocity, the arc, the Sverdrup scale, and the
 *        thickness thickness[z] or, with a cell thickness set, fixth(e3u) / fixth(e3v) at the slot's own face; 0 for the south
 *        slot of row 0
 *   q_i = w_i * d_i
 *   c_i = q_i (carry = 0), or w_i * d_i^tau (carry = 1), d^tau the slot's term of the tracer profile: fixed(.) * tf, tf the face
 *        value of the tracer of nf_field_set_tracer minus its reference, 0 for a face without a value
 *   r_i  the class row of the slot's face, 0 .. n+1 as in nf_field_compute_class_transport (n+1: no class value), from the raw
 *        face value of the class field: the class tracer when one is set, else the tracer; wrap_x is the tracer's
 *   P[r_i] += c_i where q_i > 0,   N[r_i] += c_i where q_i < 0;   q_i == 0: in neither.
 * A lane's accumulator of a row starts at +0.0 and takes its terms with z ascending and the slots in order; then the fixed tree
 * of the transect reduction follows: no atomics, bitwise reproducible.  rows (2, n + 2, row_length): P then N, each row
 * [segments | transects], written whole; a step this rank does not touch gives exact zeros.  Unlike the net class forms these
 * calls TAKE a cell thickness: P + N is the class transport (carry = 0) or the class tracer transport (carry = 1) up to
 * rounding, and the only route to them under partial steps or z* thicknesses.  Negating uo and vo gives P' == -N, N' == -P;
 * a class field equal to the level index with edges at the half-integers gives the rows of nf_field_compute_gross_profile,
 * both bit for bit.  With carry = 0, P >= 0 >= N.  The terms go through the term table of the joint class transport (40 bytes
 * x records x owned levels, allocated on first use, an error that names the size when it cannot be; the joint_window and
 * joint_skip knobs apply).  carry other than 0 or 1: NF_ERR_ARG.  Host-resident uo / vo, tracers and time-varying cell
 * thickness are staged per step.  The calls change neither the resident planes, |.| arrays, running max, last row, tracer
 * planes, class or joint state nor a captured pass. */
int nf_field_compute_gross_class_transport(nf_field **self, long tIndex, int carry, double *rows_host);       /* (2, n+2, row_length): P, N */
int nf_field_compute_gross_class_transport_async(nf_field **self, long tIndex, int carry, double *rows_dev);  /* HBM, field's stream */
/* Section area in tracer classes: the area of the section that every class occupies, and the area-weighted tracer in it --
 * the pseudo-depth axis of an overturning streamfunction in density space, the mean theta of a sigma class, and the A and T rows
 * that split the transport of a tracer into throughflow, overturning and gyre parts in class space instead of by level.  Needs
 * nf_field_set_tracer and nf_field_set_class_edges (else NF_ERR_STATE, as nf_field_compute_class_transport).  One time step t
 * over the owned levels; for every weight record and every slot i, in the order south, east, north, west:
 *   alpha_i, beta_i  the slot's area term and tracer term of nf_field_compute_area_profile: alpha = |w_i| * (th_i * arc_i) where
 *        the face counts -- its velocity is present, the tracer of nf_field_set_tracer has a finite face value x, the slot is
 *        not the south slot of row 0 -- and beta = alpha * (x - ref); th_i = thickness[z] or, with a cell thickness set,
 *        fixth(e3u) / fixth(e3v) at the slot's own face.  NO Sverdrup scale
 *   r_i  the class row of the slot's face, 0 .. n+1 as in nf_field_compute_class_transport (n+1: no class value), from the raw
 *        face value of the class field: the class tracer when one is set, else the tracer; wrap_x is the tracer's
 *   A[r_i] += alpha_i,   B[r_i] += beta_i   where the face counts; a face that does not count is in neither.
 * A lane's accumulator of a row starts at +0.0 and takes its terms with z ascending and the slots in order; then the fixed tree
 * of the transect reduction follows: no atomics, bitwise reproducible.  rows (2, n + 2, row_length): A then B, each row
 * [segments | transects], written whole; a step this rank does not touch gives exact zeros.  A >= 0.  Without a class tracer
 * row n+1 is empty: a face counts only where the tracer, which is then the class field, has a value.  The sum of A (of B) over
 * the classes is the sum over z of the A (the T) of nf_field_compute_area_profile up to rounding; a class field equal to the
 * level index with edges at the half-integers gives those rows bit for bit, and tau == ref + 1 (ref an integer) gives B == A bit
 * for bit.  The rows do not depend on the values of uo / vo, only on where they are present.  The terms go through the term
 * table of the joint class transport with TWO entries per record and owned level, the alphas and the betas (80 bytes x records
 * x owned levels, allocated on first use, an error that names the size when it cannot be; the joint_window and joint_skip knobs
 * apply, and the rows are the same bits for every setting).  Host-resident uo / vo, tracers and time-varying cell thickness are
 * staged per step.  The calls change neither the resident planes, |.| arrays, running max, last row, tracer planes, class or
 * joint state nor a captured pass. */
int nf_field_compute_class_area(nf_field **self, long tIndex, double *rows_host);       /* (2, n+2, row_length): A, B */
int nf_field_compute_class_area_async(nf_field **self, long tIndex, double *rows_dev);  /* HBM, field's stream */
/* Class tracer: a second, optional tracer at T-points (potential density sigma) that gives the faces their class value
 * instead of the tracer of nf_field_set_tracer, which is then only carried (heat by density class).  Same (nt,nz,ny,nx) and
 * dtype as uo/vo (else NF_ERR_ARG, the message naming both; set_uv first: NF_ERR_STATE); host (staged per step into a buffer
 * of its own, owned levels only) or HBM; its own two missing markers; no reference; wrap_x is the tracer's.  When it is set,
 * nf_field_compute_class_transport* bin by it too (MOC(sigma) and heat-by-sigma from one setup); tracer == NULL goes back to
 * "the class field is the tracer" and forgets the markers.  Setting the tracer itself here, with its markers, gives the rows
 * of not setting it, bit for bit.  The setters change neither a captured pass nor any resident array. */
int nf_field_set_class_tracer(nf_field **self, const void *tracer, long nt, int dtype, int on_device, double fill_value);
int nf_field_set_class_tracer_missing_value(nf_field **self, double missing_value);  /* NaN = none */
/* Tracer transport in classes: the rows of nf_field_compute_class_transport with every term times tf of the carried tracer at
 * its own face; the row is chosen by the class field (the class tracer when set, else the tracer itself, without its
 * reference).  A face whose carried tracer is missing on both sides adds 0 to the row of its class.  Same accumulation order
 * (levels ascending, slots south, east, north, west), windows and reduction as the volume form: no atomics, bitwise
 * reproducible, independent of the window; class field = level index with edges -0.5, 0.5, ... gives the tracer profile bit
 * for bit, and the sum of all rows is the tracer row up to rounding.  Owned levels only; steps this rank does not touch get
 * exact zeros.  Compute before set_tracer or set_class_edges: NF_ERR_STATE.  None of the calls of this block changes the
 * resident planes, |.| arrays, running max, last row, tracer planes or a captured pass. */
int nf_field_compute_class_tracer_transport(nf_field **self, long tIndex, double *rows_host);        /* (nedges+2, row_length) */
int nf_field_compute_class_tracer_transport_async(nf_field **self, long tIndex, double *rows_dev);   /* HBM, field's stream */
/* Conservative (piecewise-linear) remapping of the class transport: the rows of nf_field_compute_class_transport (carry = 0)
 * or nf_field_compute_class_tracer_transport (carry = 1) with every term t = w * d -- the same term, of one weight slot of one
 * record at one level z -- spread over the classes instead of going whole to the row of its face.  The class field is taken
 * to vary linearly between the layer's interfaces: with f_z the class value of the slot's face at level z (as above),
 *   g_up = 0.5 (f_{z-1} + f_z) when z > 0 and the same face has a class value at level z - 1, else f_z;
 *   g_dn = 0.5 (f_{z+1} + f_z) when z < nz - 1 and it has one at level z + 1, else f_z;
 *   lo = min(g_up, g_dn), hi = max(g_up, g_dn); for every row j from row(lo) to row(hi):
 *   left = lo in row(lo), else e[j-1]; right = hi in row(hi), else e[j]; the row gets t * ((right - left) / (hi - lo)),
 *   nothing where right == left.
 * lo == hi: whole to row(lo).  g_up, g_dn or g_dn - g_up not finite: whole to row(f_z), the step rule.  No class value at level
 * z (or NaN): whole to row n + 1.  The fractions of a term add up to 1 up to rounding, so the rows add up to the rows of the
 * step rule; a class field that is constant in z gives those rows bit for bit.  Per lane the additions run level-ascending,
 * then in slot order, then row-ascending; windows and reduction as in the step forms: no atomics, bitwise reproducible,
 * independent of the window.  Levels z - 1 and z + 1 are levels of the array, not of the owned range: under a slab range the
 * first and the last owned level read one level this rank does not own, and a host-resident class field is staged with that
 * one level more on each side (an HBM one is read in place), so sharded ranks' rows add up to the unsharded ones up to
 * rounding.  Class edges, tracer slots, window knob, scratch, state checks and refusals (NF_ERR_STATE before set_tracer or
 * set_class_edges and while a cell thickness is set) are those of nf_field_compute_class_tracer_transport; carry other than
 * 0 or 1: NF_ERR_ARG.  Changes nothing else. */
int nf_field_compute_class_remap(nf_field **self, long tIndex, int carry, double *rows_host);        /* (nedges+2, row_length) */
int nf_field_compute_class_remap_async(nf_field **self, long tIndex, int carry, double *rows_dev);   /* HBM, field's stream */
/* Remapped gross class transports: the inflow and the outflow of every class by conservative remapping -- the parts of
 * nf_field_compute_gross_class_transport at the resolution in class space of nf_field_compute_class_remap, with the scalar or a
 * per-cell thickness.  Needs nf_field_set_tracer and nf_field_set_class_edges (else NF_ERR_STATE).  One time step t over the
 * owned levels; for every weight record, owned level z and slot i, in the order south, east, north, west:
 *   q_i = w_i * d_i, d_i the slot's water term of nf_field_compute_gross_profile: the masked velocity, the arc, the Sverdrup
 *        scale, and the thickness thickness[z] or, with a cell thickness set, fixth(e3u) / fixth(e3v) at the slot's own face; 0
 *        for the south slot of row 0
 *   c_i = q_i (carry = 0), or w_i * d_i^tau (carry = 1), d^tau the slot's term of the tracer profile as in
 *        nf_field_compute_gross_class_transport; 0 for a face without a carried value
 *   c_i is spread over the class rows exactly by the rule of nf_field_compute_class_remap: g_up and g_dn from the class field
 *        (the class tracer when one is set, else the tracer; wrap_x is the tracer's) at levels z - 1 and z + 1 of the array on
 *        the same face, lo = min, hi = max, row j of row(lo) .. row(hi) gets c_i * ((right - left) / (hi - lo)), nothing where
 *        right == left; lo == hi: whole to row(lo); g_up, g_dn or g_dn - g_up not finite: whole to row(f_z); no class value at
 *        level z (or NaN): whole to row n + 1
 *   the shares go to the rows of P where q_i > 0 and to the rows of N where q_i < 0; q_i == 0 (or NaN): to neither.
 * rows (2, n + 2, row_length): P then N, each row [segments | transects], written whole.  A lane's accumulator of a row starts
 * at +0.0 and takes its shares level-ascending, then in slot order, then row-ascending; then the fixed tree of the transect
 * reduction follows: no atomics, bitwise reproducible, independent of the window (the class_window knob applies; each part is
 * built from windows of its own rows).  Hence, bit for bit: a class field that is constant in z gives the rows of
 * nf_field_compute_gross_class_transport; the level index with edges at the half-integers gives the rows of
 * nf_field_compute_gross_profile; negating uo and vo gives P' == -N, N' == -P; tau == ref + 1 gives the carry = 0 rows.  With
 * carry = 0, P >= 0 >= N.  P + N is the row set of nf_field_compute_class_remap up to rounding, and these calls TAKE a cell
 * thickness: their P + N is the route to the remapped class transports under partial steps or z* thicknesses.  Levels z - 1 and
 * z + 1 are levels of the array, not of the owned range: under a slab range a rank reads one class-field level beyond each end
 * of its levels, and a host-resident class field is staged with that halo (an HBM one is read in place); the thickness is read
 * at the owned levels only.  A step this rank does not touch gives exact zeros.  carry other than 0 or 1, or a null argument:
 * NF_ERR_ARG, decided before a device is needed; before set_tracer or set_class_edges, and for a static cell thickness uploaded
 * for another shape: NF_ERR_STATE.  Host-resident uo / vo, tracers and time-varying cell thickness are staged per step.  The
 * calls change neither the resident planes, |.| arrays, running max, last row, tracer planes, class / joint / depth / surface
 * state nor a captured pass. */
int nf_field_compute_gross_class_remap(nf_field **self, long tIndex, int carry, double *rows_host);       /* (2, n+2, row_length): P, N */
int nf_field_compute_gross_class_remap_async(nf_field **self, long tIndex, int carry, double *rows_dev);  /* HBM, field's stream */
/* Per-cell layer thicknesses (partial steps, z* / variable-volume runs): the model's e3u / e3v, or thkcello on the U and V
 * grids, in place of the one number per level of nf_field_set_thickness.  e3u sits on the index of uo (the east face of cell
 * (j, i)), e3v on the index of vo: no interpolation, no neighbour.  Definition, with th_z read at the face:
 *   fixth(x) = 0 if x is NaN or one of the thickness's own two markers (compared in its dtype), else (double)x
 *   accU(c) = fma(fixth(e3u[t',z,c]), fixed(uo[t,z,c]), accU(c)), accV(c) likewise with e3v and vo, z ascending over the
 *   owned levels; t' = t for a time-varying thickness (nt_th == nt), 0 for a static one (nt_th == 1).
 * The arc lengths and signs, the Sverdrup scale, the south and west copies, the |.| arrays, the running max and the transect
 * reduction are those of the volume rows.  The tracer rows take fma(fixth(e3u), fixed(u) * tf, accU); level z's row of
 * nf_field_compute_profile takes, per slot, the thickness at the slot's own face (east e3u[c], north e3v[c], south e3v of the
 * south cell, west e3u of the west cell), so it stays the volume row of a field whose e3u, e3v are zero on every other level.
 * Bit for bit: e3u == e3v == thickness[z] everywhere gives the rows, the six resident planes, the running max, the profile and
 * the tracer rows of the field without a cell thickness; nf_field_compute_all_async rows equal the per-step rows.
 * Untouched: nf_field_set_thickness stays required (it fixes nz) and is the thickness of every form again once the cell
 * thickness is cleared; with none set every call computes what it computed before.
 * Shape (nt_th, nz, ny, nx), x fastest, nt_th == 1 or nt, in the dtype of uo / vo -- else NF_ERR_ARG, the message naming both
 * dtypes or both step counts; set_uv and set_thickness first, else NF_ERR_STATE.  on_device = 1: HBM pointers, used in place.
 * on_device = 0: a time-varying host array is staged one step at a time, owned levels only, into buffers of its own; a
 * static one is uploaded once, at the call (set_bounds first).  e3u == NULL goes back to the per-level thickness and forgets
 * the markers.  Setting or clearing invalidates a captured pass; the all-steps-in-one-launch form of small grids is not used
 * while one is set.  Refused while one is set (NF_ERR_STATE, the message saying how to clear it): the forms that do not take
 * per-cell thicknesses yet -- nf_field_compute_tracer_profile*, nf_field_compute_class_transport*,
 * nf_field_compute_class_tracer_transport* and nf_field_compute_class_remap*.  P + N of
 * nf_field_compute_gross_class_transport* is the route to the class transports under a cell thickness, and P + N of
 * nf_field_compute_gross_class_remap* the route to the remapped ones.
 * A static host array that the handle uploaded belongs to the (nz, ny, nx) in force at that call.  After an
 * nf_field_set_bounds or nf_field_set_thickness that changes that shape (the shapes are compared, not the byte counts; a
 * call that leaves the shape as it was keeps the upload valid) every compute that would read the thickness returns
 * NF_ERR_STATE, the message naming nf_field_set_cell_thickness, and launches nothing, until nf_field_set_cell_thickness is
 * called again, with arrays of the new shape or with NULL.  Borrowed arrays -- uo / vo, the tracer, the class tracer, an HBM
 * or time-varying cell thickness -- carry no shape in their calls: the caller must set them again after a change of the grid
 * or of the levels. */
int nf_field_set_cell_thickness(nf_field **self, const void *e3u, const void *e3v, long nt_th, int dtype, int on_device,
                                double fill_value);
int nf_field_set_cell_thickness_missing_value(nf_field **self, double missing_value);   /* NaN = none */
/* Transports in true-depth bins: the terms of nf_field_compute_profile (carry = 0) or of the tracer profile (carry = 1: every
 * term times tf of the tracer of nf_field_set_tracer at its own face) binned by the DEPTH of the layer at the term's own face
 * instead of by its level -- under partial steps, z* and terrain-following coordinates a level is not a depth.
 * Depth edges e[0] < ... < e[n-1], 2 <= n <= 1025, all finite, and a finite surface value `top` (the depth of the upper
 * interface of level 0).  They are a set of their own: the class edges and the joint edges are not touched.
 * For one weight slot of one record (one face) at time step t the interface depths run over ALL levels of the array:
 *   D_0 = top,   D_{z+1} = D_z + h_z   (one float64 addition per level, z ascending from 0)
 *   h_z = fixth(e3) at the slot's own face while a cell thickness is set (east e3u[c], north e3v[c], south e3v of the south
 *         cell, west e3u of the west cell; t' as in nf_field_set_cell_thickness), else thickness[z].
 * The term t = w * d of the slot at level z -- d as in nf_field_compute_profile: the thickness at the face, the Sverdrup scale
 * and the south rule included; times tf with carry = 1 -- is spread uniformly in depth over [D_z, D_{z+1}]:
 *   D_z, D_{z+1} or D_{z+1} - D_z not finite: whole to row n + 1.  Otherwise lo = min, hi = max of the two and
 *   row(x) = the number of edges <= x;  lo == hi (a zero or missing thickness: the term is +-0): whole to row(lo);  else
 *   every row j from row(lo) to row(hi) gets t * ((right - left) / (hi - lo)), left = lo in row(lo), else e[j-1];
 *   right = hi in row(hi), else e[j]; nothing where right == left.
 * Row 0: depth < e[0]; row k: e[k-1] <= depth < e[k]; row n: depth >= e[n-1]; row n + 1 stays exactly +0.0 unless an
 * interface depth is not finite.  Per lane the additions run level-ascending, then in slot order (south, east, north, west),
 * then row-ascending, into accumulators that start at +0.0; windows ("class_window" knob) and reduction as in the class
 * forms: no atomics, bitwise reproducible, independent of the window.  The fractions of a term add up to 1 up to rounding, so
 * the rows add up to the sum over z of the profile rows; with the per-level thickness and edges D_1 .. D_{nz-1} rows
 * 0 .. nz-1 are the profile rows bit for bit.  rows (n + 2, row_length), each row [segments | transects], written whole.
 * Under a slab range the terms come from the owned levels only (a step this rank does not touch gives exact zeros) but the
 * running sum still starts at level 0: the thickness of the levels above the owned ones is read too -- in HBM in place; a
 * host-resident time-varying cell thickness is staged for the levels [0, z1) of the step -- so the ranks' rows add up to the
 * unsharded ones up to rounding.  Host-resident uo / vo and tracer are staged per step, owned levels only.
 * NF_ERR_ARG: a null argument, bad edges, a `top` that is not finite, carry other than 0 or 1 -- decided before a device is
 * needed.  NF_ERR_STATE: compute before set_depth_edges, carry = 1 before set_tracer, and the stale static cell thickness of
 * nf_field_set_cell_thickness.  The calls change neither the resident planes, |.| arrays, running max, last row, tracer
 * planes, class or joint state nor a captured pass. */
int nf_field_set_depth_edges(nf_field **self, const double *edges, int nedges, double top);
int nf_field_compute_depth_transport(nf_field **self, long tIndex, int carry, double *rows_host);        /* (nedges+2, row_length) */
int nf_field_compute_depth_transport_async(nf_field **self, long tIndex, int carry, double *rows_dev);   /* HBM, field's stream */
/* Transports between surfaces: the depth bins above with edges that are 2-D fields -- the transport inside the mixed layer,
 * above an isotherm, below an ice-shelf draft, within 200 m of the sea bed (column depth minus 200).
 * Surfaces.  m surfaces, 1 <= m <= 8, each a field at T-points of shape (nt_s, ny, nx), nt_s = 1 (static) or the nt of uo / vo,
 * in the dtype of uo / vo: surfaces[k] is the base of surface k.  Values are depths, positive downward, in the units of the
 * thicknesses, measured from the origin of `top`, the depth of the upper interface of level 0 (finite).  The surfaces have
 * two missing markers of their own (fill_value, nf_field_set_depth_surfaces_missing_value; NaN = none; NaN always counts as
 * missing) and a wrap_x of their own (nf_field_set_depth_surfaces_wrap, default 1).  They are a state of their own: the
 * depth, class and joint edges do not see them; surfaces == NULL clears them.  HBM arrays (on_device = 1) are used in place; a
 * static host set is uploaded once at the call and then belongs to the (ny, nx) of that moment -- after a set_bounds of another
 * shape every compute returns NF_ERR_STATE naming nf_field_set_depth_surfaces until it is set again or cleared; a time-varying
 * host set is staged one step at a time into a buffer of the handle.
 * Face value of a surface: the class-field rule of nf_field_compute_class_transport -- both cells beside the face have a
 * value: 0.5 * (a + b) in double; one has: that one; neither: none.  East face of c = (c, c + 1), the periodic copy in the last
 * column under wrap_x; north face = (c, c + nx); the west slot is the east face of the west cell, the south slot the north
 * face of the south cell.
 * Edges of a face.  x_1 .. x_m its face values: if any has no value or is not finite every term of the face goes whole to row
 * m + 1, at every level.  Otherwise e_1 = x_1, e_k = max(e_{k-1}, x_k): a surface that rises above the one before it is taken
 * at that one, its layer has zero width there.  The edges of a face are non-decreasing, not strictly increasing.
 * Terms and spreading.  D_z, the term t = w * d (times tf with carry = 1) and the spread rule are those of
 * nf_field_compute_depth_transport with the face's own e in place of the global edges: D_0 = top, D_{z+1} = D_z + h_z from
 * level 0 under a slab range too; row(x) = the number of e_k <= x; a depth or a difference that is not finite: whole to row
 * m + 1; lo == hi: whole to row(lo); else row j gets t * ((right - left) / (hi - lo)), nothing where right == left.
 * Rows.  m + 2 rows of row_length, each [segments | transects], written whole: row 0 above surface 1, row k between surfaces
 * k and k + 1, row m below surface m, row m + 1 the faces without an edge set or with a depth that is not finite (exactly
 * +0.0 otherwise).  Per lane the additions run level-ascending, then in slot order (south, east, north, west), then
 * row-ascending, into accumulators that start at +0.0; scan and finalize as in the class forms: no atomics, bitwise
 * reproducible, independent of the "class_window" knob.  With surfaces that are constant over the grid at e_1 < .. < e_m the
 * rows are those of nf_field_compute_depth_transport with these edges, bit for bit.
 * NF_ERR_ARG, decided before a device is needed: a null argument, m outside 1 .. 8, nt_s not 1 or nt, a dtype other than that
 * of uo / vo (the message names both), a `top` that is not finite, carry other than 0 or 1.  NF_ERR_STATE: the setter before
 * set_uv, a compute before the setter, carry = 1 before set_tracer.  The calls change neither the resident planes, |.| arrays,
 * running max, last row, tracer planes, any edge set nor a captured pass. */
int nf_field_set_depth_surfaces(nf_field **self, const void *const *surfaces, int m, long nt_s, int dtype, int on_device,
                                double fill_value, double top);
int nf_field_set_depth_surfaces_missing_value(nf_field **self, double missing_value);   /* NaN = none */
int nf_field_set_depth_surfaces_wrap(nf_field **self, int wrap_x);
int nf_field_compute_surface_transport(nf_field **self, long tIndex, int carry, double *rows_host);        /* (m+2, row_length) */
int nf_field_compute_surface_transport_async(nf_field **self, long tIndex, int carry, double *rows_dev);   /* HBM, field's stream */
/* Read-back of the resident per-step arrays into caller-owned HOST arrays, in place (fluxviz.py aliases
 * them: fluxviz.py:148,160,168): integratedVelocity (ncell,4), edgeFluxesU/V (ncell) = |flux|; any may be
 * NULL.  max_abs: running max (field.py:234). */
int nf_field_read_step(nf_field **self, double *iV_host, double *eU_host, double *eV_host, double *max_abs);
int nf_field_reset_max(nf_field **self);
int nf_field_get_arclengths(nf_field **self, double *arc_host /* (ncell,4) */);
int nf_field_get_points(nf_field **self, double *points_host /* (ncell,4,3) */);
int nf_field_get_box(nf_field **self, double *lonmin, double *lonmax, double *latmin, double *latmax);
/* HBM addresses of resident arrays (for zero-copy consumers / RCCL): which = 0 integratedVelocity,
 * 1 |eU|, 2 |eV|, 3 arcLengths (ncell,4), 4 corner table (ncell,4,2) */
int nf_field_device_ptr(nf_field **self, int which, void **dev);
/* A Grid_t view of the field's corner table (so mint.PolylineIntegral objects can share it). */
int nf_field_grid(nf_field **self, Grid_t **grid);
/* Kernel timing with HIP events on the field's stream, around the vertical-integral+edge-flux launches
 * (bench.py's roofline leg): enable, run, then read (launch count, total ms).  enable > 1 also creates that many
 * event triples up front, so that no event is created inside a timed region; the events are re-used after every read
 * (at most 65536 launches are recorded between two reads). */
int nf_field_timing(nf_field **self, int enable);
int nf_field_timing_read(nf_field **self, long *launches, double *total_ms);
/* how the total of the last nf_field_timing_read splits between the flux kernel and the expansion kernel behind it */
int nf_field_timing_split(nf_field **self, double *flux_ms, double *expand_ms);
/* time of the transect reductions (K3: gather + segmented scan + the two finalize kernels) launched behind the timed flux
 * launches of the last nf_field_timing_read -- measured with the same events, not part of its total */
int nf_field_timing_k3(nf_field **self, double *k3_ms);

/* ------------------------------------------------------------------ multi-GPU: the one collective */
/* The reference walks the time steps serially (fluxplot.py:51-59) and contracts z with one tensordot (field.py:161); here
 * every rank integrates its own (t,z) slabs (nf_field_set_slab_range above) into partial rows (nt, row_length) and ONE
 * all-reduce(sum, float64) over RCCL / xGMI gives every rank the totals.  One process per GPU.  librccl is resolved at
 * first use from the copy the process already holds (PyTorch's, or the system's librccl.so.1): no link-time dependency.
 *   nf_rccl_unique_id : rank 0 creates the 128-byte id and hands it to the other ranks by any means (file, socket, MPI,
 *                       torch.distributed store)
 *   nf_rccl_preflight : NOT collective: checks what nf_rccl_comm_init needs that does not involve the other ranks (librccl
 *                       resolves, the calling thread has a usable HIP device; *device = its index).  ncclCommInitRank is
 *                       collective, so a rank that failed before it would leave the others waiting inside it: call this
 *                       on every rank, agree on the outcome over the channel that carried the id, then init together
 *   nf_rccl_comm_init : every rank, after nf_set_device(its GPU); collective over the nranks callers
 *   nf_rows_allreduce : rows_dev (HBM, n doubles) summed in place over all ranks, asynchronous on hip_stream.  rccl_comm may
 *                       also be a ncclComm_t the caller created itself with the same librccl
 *   nf_rccl_comm_info : what the communicator says about itself (number of ranks, this rank, HIP device index)
 *   nf_rccl_library   : path of the librccl the entry points were resolved from */
#define NF_RCCL_UNIQUE_ID_BYTES 128
int nf_rccl_unique_id(void *id128);
int nf_rccl_preflight(int *device);
int nf_rccl_comm_init(void **comm, int nranks, const void *id128, int rank);
int nf_rccl_comm_destroy(void *comm);
int nf_rccl_comm_info(void *comm, int *nranks, int *rank, int *device);
int nf_rccl_library(char *buf, int buflen);
int nf_rows_allreduce(void *rccl_comm, double *rows_dev, size_t n, void *hip_stream);

/* ------------------------------------------------------------------ file ingest straight to HBM (field.py:149) */
/* Real NEMO files are NetCDF-4 = HDF5 with uo / vo stored as byte-shuffled, deflated chunks; the reference has netCDF4 /
 * xarray inflate one time step on the host at every update (field.py:149: nc[name][timeIndex, :, :, :]).  Here the
 * compressed chunks are handed over as they sit in the file and are inflated on the device, one wavefront per chunk
 * (RFC 1950/1951 decoder with the Adler-32 check, then the inverse of HDF5's shuffle filter), into out_dev.
 *   comp_host  : host buffer (pinned for an asynchronous copy) holding the compressed chunks, comp_bytes long; NULL = the
 *                bytes a preceding nf_inflater_upload of the same comp_bytes put in HBM
 *   in_off/in_len[i] : where chunk i's zlib stream sits in comp_host
 *   chunk_bytes      : decoded size of every chunk = cz*cy*cx*elem_size (checked against what each stream inflates to)
 *   elem_size        : 4 or 8 (1 for raw bytes); shuffled != 0: the chunks went through HDF5's shuffle filter
 *   chunk_dims (3)   : (cz, cy, cx) of a chunk; slab_dims (3): (nz, ny, nx) of the time step; origin (nchunks x 3): where
 *                      each chunk starts in the slab -- chunks may tile y and x, edge chunks may hang over the slab
 *   out_dev          : the slab in HBM, nz*ny*nx*elem_size bytes
 *   status_host (nchunks ints or NULL): 0 = fine, else the decoder's error code per chunk
 * Synchronous on hip_stream.  NF_ERR_ARG (message names the first bad chunk) if any stream is malformed -- the slab is
 * then undefined; nothing outside it is ever written. */
typedef struct nf_inflater nf_inflater;
int nf_inflater_new(nf_inflater **self);
int nf_inflater_del(nf_inflater **self);
/* `self` uses owner's decode scratch (the decoded group, job and status arrays) from now on instead of its own: for two
 * inflaters whose nf_inflater_run calls never overlap in time (a run is synchronous) but which each need their own
 * compressed buffer -- the two staging slots of a file-backed field.  owner must outlive self. */
int nf_inflater_share_scratch(nf_inflater **self, nf_inflater **owner);
/* how many chunks the device decodes at once (resident decoder wavefronts): callers batch that many per nf_inflater_run */
int nf_inflater_capacity(int *streams);
/* Early upload: copy comp_bytes of compressed chunks to HBM on the inflater's own stream, complete at return.  Meant for a
 * staging thread that has just gathered the NEXT group while the GPU still decodes this one (the copy then runs under the
 * decode); a following nf_inflater_run with comp_host = NULL and the same comp_bytes decodes what was uploaded. */
int nf_inflater_upload(nf_inflater **self, const void *comp_host, size_t comp_bytes);
/* The same straight from the mapped file, without a staging copy: range i (src_addr[i], len[i] bytes of ordinary host memory)
 * goes to byte dst_off[i] of the compressed buffer of comp_bytes bytes; what lies between the ranges reads as zeros. */
int nf_inflater_upload_ranges(nf_inflater **self, const unsigned long long *src_addr, const long long *dst_off,
                              const long long *len, long long n, size_t comp_bytes);
int nf_inflater_run(nf_inflater **self, const void *comp_host, size_t comp_bytes, const long long *in_off,
                    const long long *in_len, int nchunks, long long chunk_bytes, int elem_size, int shuffled,
                    const long long *chunk_dims, const long long *slab_dims, const long long *origin, void *out_dev,
                    void *hip_stream, int *status_host);
/* The same into a STACK of slabs: out_dev holds slab_dims[0] / stack_nz slabs of (stack_nz, ny, nx) one behind the other
 * (the variables and time steps of a group, decoded by one launch), origin[3 i] counts levels from the top of the stack.  A
 * chunk that hangs over in z is cut at the end of the slab it starts in: the levels behind it belong to the next slab.
 * stack_nz = 0 (what nf_inflater_run passes): one slab.  slab_dims[0] must be a multiple of stack_nz. */
int nf_inflater_run_stacked(nf_inflater **self, const void *comp_host, size_t comp_bytes, const long long *in_off,
                            const long long *in_len, int nchunks, long long chunk_bytes, int elem_size, int shuffled,
                            const long long *chunk_dims, const long long *slab_dims, const long long *origin, void *out_dev,
                            void *hip_stream, int *status_host, long long stack_nz);
/* Which placement launch nf_inflater_run takes for a chunk geometry (it asks this very function): BYTES = raw bytes;
 * PLANES16_F4 / PLANES4_* = shuffled chunks of whole (y, x) planes, 16 or 4 elements per lane; ROWS4_* = other shuffled chunks
 * whose rows are a multiple of four elements long, 4 per lane; ELEM_* = one element per lane.  Needs no GPU: the tests'
 * geometry table is checked against it, so that a change of the dispatch cannot drop a launch from the suite unnoticed. */
enum {
    NF_PLACE_BYTES = 0,
    NF_PLACE_PLANES16_F4 = 1,
    NF_PLACE_PLANES4_F4 = 2,
    NF_PLACE_PLANES4_F8 = 3,
    NF_PLACE_ROWS4_F4 = 4,
    NF_PLACE_ROWS4_F8 = 5,
    NF_PLACE_ELEM_F4_SHUFFLED = 6,
    NF_PLACE_ELEM_F4 = 7,
    NF_PLACE_ELEM_F8_SHUFFLED = 8,
    NF_PLACE_ELEM_F8 = 9,
    NF_PLACE_FORMS = 10
};
int nf_inflater_place_form(int elem_size, int shuffled, const long long *chunk_dims, const long long *slab_dims, int *form);

/* ------------------------------------------------------------------ time means (nf_timemean.hip) */
/* The time mean of nsteps arrays of n values each, step t at src_dev + t * stride_elems elements of dtype (HBM).  Per value
 * i, the steps visited strictly in ascending order:
 *     s = +0.0, c = 0                  (first = 0: the s, c that the previous call left in acc_dev / cnt_dev)
 *     x = src[t * stride_elems + i];   x present:  s = s + (double)x, c += 1
 * Present: not NaN and equal to neither marker, each marker cast to dtype and compared in dtype (fill, missing: NaN = none);
 * +-inf is present.  No other arithmetic, no reassociation: a series split over several calls (first on the first one only,
 * last on the last one only) gives the bits of one call, whatever the launch shape.
 * last = 0: acc_dev[i] = s, cnt_dev[i] = c for the next call.  last = 1: acc_dev[i] becomes the mean,
 *     NF_MEAN_OVER_STEPS    s / total_steps   (the velocity rule: a missing velocity counts as 0, as in every flux kernel)
 *     NF_MEAN_OVER_PRESENT  s / c             (the tracer rule)
 * and fill_out where c == 0, under both rules; total_steps is read by that call only.
 * cnt_dev may be NULL when first && last (nothing is carried: nsteps * n * sizeof(dtype) bytes in, 8 n bytes out).
 * NF_ERR_ARG, decided before a device is needed: NULL acc_dev / src_dev, nsteps < 1, n == 0, stride_elems < n with
 * nsteps > 1, a bad dtype or rule, last with NF_MEAN_OVER_STEPS and total_steps < 1, NULL cnt_dev without first && last.
 * Asynchronous on hip_stream. */
#define NF_MEAN_OVER_STEPS 0
#define NF_MEAN_OVER_PRESENT 1
int nf_time_mean(double *acc_dev, unsigned *cnt_dev, const void *src_dev, long nsteps, long long stride_elems, size_t n,
                 int dtype, double fill, double missing, int first, int last, int rule, long total_steps, double fill_out,
                 void *hip_stream);
/* The thickness-weighted time mean of a velocity series and the mean of the cell thickness at its points (z*, variable-volume
 * output): nsteps arrays of n values each of both, step t at src_dev + t * src_stride_elems and thk_dev + t * thk_stride_elems
 * elements of dtype (HBM).  Per value i, the steps visited strictly in ascending order:
 *     sF = +0.0, sH = +0.0, c = 0              (first = 0: what the previous call left in accf_dev / acch_dev / cnt_dev)
 *     h = fixth(thk[t * thk_stride_elems + i]) fixth as in nf_field_set_cell_thickness: NaN or one of the thickness's two
 *                                              markers (thk_fill, thk_missing, compared in dtype) -> 0, else (double)
 *     sH = sH + h                              at every step
 *     x = src[t * src_stride_elems + i];       x present (nf_time_mean's rule with fill, missing):
 *                                              sF = sF + (h * (double)x), c += 1     the product rounded, then added: no fma
 * No other arithmetic, no reassociation: a series split over several calls gives the bits of one call, whatever the launch
 * shape, as for nf_time_mean.
 * last = 0: accf_dev[i] = sF, acch_dev[i] = sH, cnt_dev[i] = c for the next call.  last = 1:
 *     accf_dev[i] = c == 0 ? fill_out : (sH == 0 ? +0.0 : sF / sH)     the weighted mean velocity
 *     acch_dev[i] = sH / total_steps                                   the mean thickness
 * so that (mean thickness) x (mean velocity) is the mean of thickness x velocity, face by face, up to rounding; a velocity
 * missing at every step stays missing, water that is never there (sH == 0) gives velocity 0 and thickness 0.
 * cnt_dev may be NULL when first && last (nothing is carried: 2 * nsteps * n * sizeof(dtype) bytes in, 16 n bytes out).
 * NF_ERR_ARG, decided before a device is needed: NULL accf_dev / acch_dev / src_dev / thk_dev, nsteps < 1, n == 0, either
 * stride < n with nsteps > 1, a bad dtype, last with total_steps < 1, NULL cnt_dev without first && last.
 * Asynchronous on hip_stream. */
int nf_time_mean_weighted(double *accf_dev, double *acch_dev, unsigned *cnt_dev, const void *src_dev, long long src_stride_elems,
                          const void *thk_dev, long long thk_stride_elems, long nsteps, size_t n, int dtype, double fill,
                          double missing, double thk_fill, double thk_missing, int first, int last, long total_steps,
                          double fill_out, void *hip_stream);
/* The two means above over selected, weighted steps: a table of nsteps steps, step j at src_dev + step_offsets[j] elements of
 * dtype (HBM) with the weight weights[j] (step lengths: the months of an annual mean).  step_offsets and weights are HOST
 * arrays, read before the call returns; weights = NULL: all 1.  The offsets are >= 0, in any order, and may repeat.  Per
 * value i, the table walked strictly in order j = 0 .. nsteps - 1, everything float64, no fma, no reassociation:
 *     x = src[step_offsets[j] + i];   x present (nf_time_mean's rule):
 *                                     s = s + (w_j * (double)x), wp = wp + w_j, c += 1     the product rounded, then added
 * first = 0: s, wp, c start from acc_dev / wsum_dev / cnt_dev as the previous call left them.  last = 1: acc_dev[i] becomes
 *     NF_MEAN_OVER_STEPS    s / total_weight
 *     NF_MEAN_OVER_PRESENT  s / wp
 * and fill_out where c == 0.  total_weight is the caller's float64 sum of all weights of all calls, added in order; it is
 * read by the last call only.  Any cut of a table into calls gives the bits of one call.  Unit weights (or NULL) on the offsets
 * j * stride_elems with total_weight = total_steps give the bits of nf_time_mean (1 * x is exact, wp == c); so do weights
 * that all equal one power of two.
 * wsum_dev is read and written under NF_MEAN_OVER_PRESENT only; it may be NULL under NF_MEAN_OVER_STEPS or when first && last,
 * and so may cnt_dev when first && last.  When any listed step, acc_dev, wsum_dev or cnt_dev is not 16-byte aligned the whole
 * call takes one value per lane: the same bits.  The table travels as kernel arguments, 16 steps a launch; a longer table is
 * a chain of launches that carries acc, cnt (and wsum) between them, 12 n (20 n) bytes each way per further launch.
 * NF_ERR_ARG, decided before a device is needed: NULL acc_dev / src_dev / step_offsets, nsteps < 1, n == 0, a bad dtype or
 * rule, a negative offset, a weight that is not finite and > 0, last with NF_MEAN_OVER_STEPS and a total_weight that is not
 * finite and > 0, a NULL cnt_dev or wsum_dev where it is not allowed.  Asynchronous on hip_stream. */
int nf_time_mean_steps(double *acc_dev, double *wsum_dev, unsigned *cnt_dev, const void *src_dev, const long long *step_offsets,
                       const double *weights, long nsteps, size_t n, int dtype, double fill, double missing, int first, int last,
                       int rule, double total_weight, double fill_out, void *hip_stream);
/* nf_time_mean_weighted over selected, weighted steps: step j of the velocity at src_dev + src_offsets[j], of the thickness
 * at thk_dev + thk_offsets[j] elements.  Per value i, the table walked strictly in order:
 *     g = w_j * fixth(thk[thk_offsets[j] + i])    rounded
 *     sH = sH + g                                 at every step
 *     x = src[src_offsets[j] + i];  x present:    sF = sF + (g * (double)x), c += 1       the product rounded, then added
 * last = 1: accf_dev[i] = c == 0 ? fill_out : (sH == 0 ? +0.0 : sF / sH), acch_dev[i] = sH / total_weight.  Everything else
 * as for nf_time_mean_steps (there is no wsum_dev; a further launch of a chain carries 28 n bytes each way); unit weights on
 * the offsets j * stride give the bits of nf_time_mean_weighted. */
int nf_time_mean_weighted_steps(double *accf_dev, double *acch_dev, unsigned *cnt_dev, const void *src_dev,
                                const long long *src_offsets, const void *thk_dev, const long long *thk_offsets,
                                const double *weights, long nsteps, size_t n, int dtype, double fill, double missing,
                                double thk_fill, double thk_missing, int first, int last, double total_weight, double fill_out,
                                void *hip_stream);

/* Potential density anomaly sigma_pref(theta, S) = rho(S, T_pref, pref) - 1000 in kg m-3 by the UNESCO EOS-80 equation of state,
 * value by value over n values of dtype in HBM (nf_eos.hip): theta_dev potential temperature in degC referenced to the surface,
 * salt_dev practical salinity, pref_dbar the reference pressure in dbar, uniform over the call.  pref_dbar == 0: T_pref = theta
 * and rho is the one-atmosphere equation (sigma0).  pref_dbar > 0: T_pref is theta moved adiabatically from 0 to pref_dbar by the
 * Fofonoff-Millard Runge-Kutta step over Bryden's lapse rate, rho the one-atmosphere density over 1 - P / K with the secant bulk
 * modulus K (sigma2, sigma4).  All arithmetic is float64 in the operation order written in nf_eos.hip, without fused
 * multiply-adds; float32 inputs are widened first, the result is rounded once to dtype.  TEOS-10 (conservative temperature,
 * absolute salinity) is not covered.
 * A value is present when it is not NaN and equals neither of its array's two markers (theta_fill, theta_missing; salt_fill,
 * salt_missing; NaN = none), each cast to dtype and compared in dtype.  Where theta or S is missing out_dev gets fill_out (cast to
 * dtype).  A negative S gives NaN.  3 * n * sizeof(dtype) bytes move.  n == 0 is a no-op.
 * NF_ERR_ARG, decided before a device is needed: a bad dtype, pref_dbar negative or not finite, and with n > 0 a NULL pointer or
 * an out_dev that overlaps theta_dev or salt_dev without being equal to it (in place over either input is allowed).
 * Asynchronous on hip_stream. */
int nf_sigma_eos80(void *out_dev, const void *theta_dev, const void *salt_dev, size_t n, int dtype, double pref_dbar,
                   double theta_fill, double theta_missing, double salt_fill, double salt_missing, double fill_out,
                   void *hip_stream);

/* The depth at which a tracer first reaches a value, column by column (nf_isodepth.hip): the depth of an isotherm or an
 * isopycnal, the mixed-layer depth by a threshold criterion -- the surfaces of nf_field_set_depth_surfaces, computed from what
 * the model writes.  Value-level like nf_sigma_eos80: no nf_field involved, asynchronous on hip_stream.
 * Inputs.  tau_dev: one time step of a tracer at T-points, (nz, ny, nx), x fastest, of dtype in HBM, with two missing markers
 * (tau_fill, tau_missing; NaN = none; NaN always counts as missing; each cast to dtype and compared in dtype).  The thicknesses
 * of the levels: either thickness_host, nz float64 numbers on the host, one per level, read before the call returns (at most
 * 256 levels), or e3t_dev, (nz, ny, nx) of dtype in HBM with two markers of its own (e3t_fill, e3t_missing) -- exactly one of
 * the two is not NULL.  top: the depth of the upper interface of level 0, finite.  values: m float64 numbers on the host,
 * 1 <= m <= 8, read before the call returns.  sense: +1, the tracer rises downward (density), or -1, it falls (temperature).
 * Output.  out_dev: m planes (m, ny, nx) of dtype, plane j the depth of values[j], positive downward from the origin of top.
 * All arithmetic is float64, every operation rounded on its own, no fused multiply-adds; float32 inputs are widened first and a
 * result is rounded once to dtype.  Per column, tau_k and h_k its values at level k:
 *   Wet levels.  Level k is wet when tau_k is present and, in the e3t form, h_k is present, finite and > 0.  The column is the
 *     leading run of wet levels 0 .. kb; what lies below the first level that is not wet does not matter (at most one group
 *     of 4 or 8 levels below it is still read).  No wet level: every plane gets fill_out.  (Ice-shelf cavities -- dry levels on top -- are out of scope.)
 *   Depths.  D_0 = top, D_{k+1} = D_k + h_k, c_k = D_k + 0.5 * h_k, sequentially from level 0.
 *   Threshold.  relative = 0: theta_j = values[j].  relative = 1: theta_j = tau_ref + values[j] (+0.03 kg m-3 on sigma0 with
 *     sense +1, -0.2 K on theta with sense -1, zref = 10: the mixed-layer criteria), where kref is the last level of the column
 *     with c_k <= zref (0 if there is none) and tau_ref = tau_kref when zref <= c_0 or kref = kb, else, with a = kref and
 *     b = kref + 1, tau_ref = tau_a + (tau_b - tau_a) * ((zref - c_a) / (c_b - c_a)), in that operation order.
 *   Reached.  R_k = tau_k >= theta_j (sense +1) or tau_k <= theta_j (sense -1).  k* = the first k in [k0, kb] with R_k; k0 = 0
 *     with relative = 0, kref + 1 with relative = 1.
 *   Result.  No k*: D_{kb+1}, the sea bed (the whole column is above the surface).  k* = 0: D_0, the surface outcrops.
 *     Otherwise, with a = k* - 1 and k = k*:  R_a false: c_a + (c_k - c_a) * ((theta_j - tau_a) / (tau_k - tau_a)), in that
 *     operation order;  R_a true (only with relative = 1 at a = kref): zref.  A result that is not finite (+-inf in the tracer)
 *     is stored as it comes: nf_field_compute_surface_transport sends such faces to row m + 1.
 * The result does not depend on the launch shape; no atomics.  A wave stops reading a column's levels once every lane has all
 * its m values or has left its wet column.
 * NF_ERR_ARG, decided before a device is needed: a null out_dev, tau_dev or values; both thickness forms or neither; m outside
 * 1 .. 8; a bad dtype; a sense other than +-1; relative other than 0 or 1; a top, zref or value that is not finite; nz, ny or
 * nx < 1; more than 256 levels, or a thickness that is not finite and > 0, in the thickness_host form; out_dev overlapping
 * tau_dev or e3t_dev. */
int nf_iso_depth(void *out_dev, const void *tau_dev, const double *thickness_host, const void *e3t_dev, long nz, long ny, long nx,
                 int dtype, double tau_fill, double tau_missing, double e3t_fill, double e3t_missing, double top,
                 const double *values, int m, int sense, int relative, double zref, double fill_out, void *hip_stream);

/* Layer thicknesses at the U and V faces from the thickness at T-points (nf_facethick.hip): the e3u / e3v of
 * nf_field_set_cell_thickness computed from what the model writes -- e3t in grid_T, thkcello of CMIP6 -- where grid_U / grid_V
 * carry none.  Value-level like nf_sigma_eos80 / nf_iso_depth: no nf_field involved, asynchronous on hip_stream.  All arrays
 * are (nz, ny, nx), x fastest, of dtype, in HBM: e3t_dev one time step of the T-grid thickness; e3t0_dev, e3u0_dev, e3v0_dev the
 * static thicknesses at the T, U and V points (e3t_0, e3u_0, e3v_0 of a mesh_mask), all three with NF_E3_ANOMALY, all NULL
 * otherwise; e3u_out_dev on the index of uo (the east face of cell (j, i)), e3v_out_dev on the index of vo (its north face).
 * Definition.  Everything is float64.  Every operation is rounded on its own, with no fused multiply-adds.  Inputs are widened
 * first.  Each result is rounded once to dtype.
 *   Presence.  present(x): x is not NaN and equals neither of its array's two markers, each cast to dtype and compared in
 *     dtype.  fill / missing apply to e3t; fill0 / missing0 apply to all three statics.  NaN means "no marker".
 *   Cell values.  For cell (z, j, i): A = e3t[z,j,i] and A0 = e3t0[z,j,i].
 *   East (U) face.  This is the index of uo and the neighbour rule of the tracer block above.  B = e3t[z,j,i+1].  At
 *     i = nx-1, B = e3t[z,j,0] when wrap_x is on, else no neighbour.
 *   North (V) face.  B = e3t[z,j+1,i].  At j = ny-1 there is no neighbour.
 *   Static neighbour.  B0 comes from e3t0 in the same way as B.
 *   No neighbour by geometry.  Then B := A and B0 := A0.
 *   rule = NF_E3_MIN (0; NEMO's partial-step rule e3u_0 = min(e3t_0(i), e3t_0(i+1))).  A and B both present: B < A ? B : A.
 *     Otherwise +0.0: a face beside a cell without a thickness has no open area.
 *   rule = NF_E3_MEAN (1).  Both present: 0.5 * (A + B).  Otherwise +0.0.
 *   rule = NF_E3_ANOMALY (2; the z* / vvl rule of NEMO's dom_vvl_interpol WITHOUT its cell-area weights e1e2t / e1e2u: the
 *     anomalies of the two cells count equally, which is NEMO's result only where the two cells have one area).  It needs the
 *     three statics.  F0 is e3u0[z,j,i] for the east face and e3v0[z,j,i] for the north face.  F0 not present: +0.0.  F0
 *     present and A, B, A0, B0 all present: F0 + 0.5 * ((A - A0) + (B - B0)), in that order.  F0 present but one of A, B, A0,
 *     B0 missing: F0 (NEMO keeps e3u_0 on a masked face).
 *   Non-finite or negative results are stored as they come.
 * The result does not depend on the launch shape; there are no atomics.  3 * n * sizeof(dtype) bytes move with NF_E3_MIN and
 * NF_E3_MEAN, 6 * n * sizeof(dtype) with NF_E3_ANOMALY (n = nz * ny * nx).
 * NF_ERR_ARG, decided before a device is needed: a null output pointer or a null e3t_dev; a bad dtype; a bad rule; nz, ny or
 * nx < 1; statics given with rule 0 or 1, or any of them absent with rule 2; an output that overlaps an input or the other
 * output. */
#define NF_E3_MIN 0
#define NF_E3_MEAN 1
#define NF_E3_ANOMALY 2
int nf_face_thickness(void *e3u_out_dev, void *e3v_out_dev, const void *e3t_dev, const void *e3t0_dev, const void *e3u0_dev,
                      const void *e3v0_dev, long nz, long ny, long nx, int dtype, int rule, int wrap_x, double fill,
                      double missing, double fill0, double missing0, void *hip_stream);

/* z* layer thicknesses at the U and V faces from the sea surface height (nf_sshthick.hip): the e3u / e3v of
 * nf_field_set_cell_thickness for ln_vvl_zstar / key_qco / key_linssh output, which holds the 2-D ssh / zos and a static
 * mesh_mask and no 3-D thickness: e3u(t) = e3u_0 * (1 + ssh_u(t) / hu_0).  Both calls are value-level like nf_face_thickness:
 * no nf_field involved, asynchronous on hip_stream.  All arrays are in HBM, x fastest: ssh_dev one (ny, nx) plane of dtype, one
 * time step of the sea surface height at T-points; e3u0_dev / e3v0_dev the static thicknesses at the U and V points (e3u_0,
 * e3v_0 of a mesh_mask), (nz, ny, nx) of dtype, as are the outputs, e3u_out_dev on the index of uo (the east face of cell
 * (j, i)) and e3v_out_dev on the index of vo (its north face); hu0_dev / hv0_dev the column depths at the U and V points,
 * (ny, nx) float64 -- a mesh file's hu_0 / hv_0 or nf_column_depth of the two statics; area_t_dev, area_u_dev, area_v_dev the
 * cell areas e1e2t, e1e2u, e1e2v, (ny, nx) float64, all three or all NULL.
 * Definition.  Everything is float64.  Every operation is rounded on its own, with no fused multiply-adds.  Inputs are widened
 * first.  Each result is rounded once to dtype.
 *   Presence.  present(x): x is not NaN and equals neither of its array's two markers, each cast to dtype and compared in
 *     dtype.  fill / missing apply to ssh; fill0 / missing0 apply to the two statics.  NaN means "no marker".
 *   Column depth (nf_column_depth).  H = +0.0.  For k = 0 ... nz-1 in that order, H = H + (double)F0[k,j,i] where F0[k,j,i] is
 *     present.  Values are added as they come, including negative or non-finite ones.
 *   Neighbours.  Those of nf_face_thickness.  East (U) face of (j, i): Sa = ssh[j,i], Sb = ssh[j,i+1].  At i = nx-1,
 *     Sb = ssh[j,0] when wrap_x is on, else no neighbour.  North (V) face: Sb = ssh[j+1,i].  At j = ny-1 there is no neighbour.
 *   No neighbour by geometry.  Then Sb := Sa, and with areas the neighbour's area becomes the cell's own.
 *   Face height s, without areas.  0.5 * (Sa + Sb) when both are present, else +0.0.
 *   Face height s, with areas (NEMO's ssh_u = 1/2 (e1e2t_i ssh_i + e1e2t_i+1 ssh_i+1) / e1e2u).  p = Ta * Sa and q = Tb * Sb,
 *     where Ta, Tb are area_t at the two cells.  s = (0.5 * (p + q)) / F, where F is area_u[j,i] or area_v[j,i].  s = +0.0
 *     when Sa or Sb is missing, when any of Ta, Tb, F is NaN, or when F is not > 0.
 *   Factor.  H is hu0[j,i] for the east face and hv0[j,i] for the north face.  r = s / H when H > 0, else +0.0; a NaN H also
 *     gives +0.0.  Then f = 1.0 + r.
 *   Result per level.  F0 is e3u0[k,j,i] for the east face and e3v0[k,j,i] for the north face.  +0.0 where F0 is not present,
 *     else (dtype)((double)F0 * f).  Non-finite or negative results are stored as they come.
 * The result does not depend on the launch shape; there are no atomics.  nf_ssh_thickness moves 4 * n * sizeof(dtype) bytes
 * (n = nz * ny * nx) plus the planes.
 * NF_ERR_ARG, decided before a device is needed: a null output, ssh_dev, static or column-depth pointer; one or two of the
 * three area pointers given; a bad dtype; nz, ny or nx < 1; nz * ny * nx overflowing; an output that overlaps any input or the
 * other output. */
int nf_column_depth(double *h_out_dev, const void *e3_0_dev, long nz, long ny, long nx, int dtype, double fill0,
                    double missing0, void *hip_stream);
int nf_ssh_thickness(void *e3u_out_dev, void *e3v_out_dev, const void *ssh_dev, const void *e3u0_dev, const void *e3v0_dev,
                     const double *hu0_dev, const double *hv0_dev, const double *area_t_dev, const double *area_u_dev,
                     const double *area_v_dev, long nz, long ny, long nx, int dtype, int wrap_x, double fill, double missing,
                     double fill0, double missing0, void *hip_stream);

/* ------------------------------------------------------------------ synthetic data (datagen.py) */
/* Stream functions offered on device (no eval on the GPU): psi = g(z,t) * h(x,y)
 *   0 "x"                                                    README.md:26
 *   1 "arctan2(y, x+180)/(2*pi)"                             README.md:50
 *   2 "cos(2*pi*y/360) + sin(2*pi*x/360)"                    README.md:65
 *   3 "(1+10*z)*(t+1)*(cos(2*pi*y/360) + sin(2*pi*x/360))"   README.md:89
 *   4 "(cos(t*2*pi/nt)+2)*(0.5*(y/180)**2 + sin(2*pi*x/360))" datagen.py:211 (default)
 *   5 "(1+10*z)*(t+1)*arctan2(y, x+180)/(2*pi)"              (config C4's modulated singular case) */
#define NF_PSI_COUNT 6
/* datagen.py:42-66 (+ rotatePole :116-166 when deltaDeg != (0,0)): writes bounds_lon/lat (ny,nx,4) f64
 * into HBM.  lat_uses_dx=1 reproduces datagen.py:49 (latitude spaced with dx). */
int nf_datagen_bounds(double *bounds_lon_dev, double *bounds_lat_dev, long ny, long nx, double xmin,
                      double xmax, double ymin, double ymax, double delta_lon_deg, double delta_lat_deg,
                      int lat_uses_dx, void *hip_stream);
/* datagen.py:69-113 for time steps [t_begin, t_end): writes u,v ((t_end-t_begin),nz,ny,nx) of dtype into
 * HBM; nt is the series length (enters psi 4).  zhalf_k = zmin+(k+0.5)dz. */
int nf_datagen_uv(void *u_dev, void *v_dev, int dtype, long t_begin, long t_end, long nt, long nz, long ny,
                  long nx, double xmin, double xmax, double ymin, double ymax, double zmin, double zmax,
                  int lat_uses_dx, int psi, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* NEMOFLUX_AMD_H */
