"""Headless time series of the flux across one or more transects: the batch driver of nemoflux/fluxplot.py:18-76.

The reference loops `for itime in range(nt): fld.update(); pli.getIntegral(...)` (fluxplot.py:51-59), one host round
trip per step and per transect.  Here ALL time steps and ALL transects are integrated in one asynchronous pass on
the GPU (Field.computeAll) and only the (nt, ntransect) table comes back.  Plotting uses matplotlib (imported
only with --show): the table is always printed or written as CSV, which is what the plot shows.

    python -m nemoflux_amd.fluxplot -t T.npz -u U.npz -v V.npz -l "[(-100,-80),(100,-80),(0,80)],[...]" [-s] [-o out.csv]
    python -m nemoflux_amd.fluxplot -t T.npz -u U.npz -v V.npz -i "data/nz/*.txt"
    python -m nemoflux_amd.fluxplot -t T.npz -u U.npz -v V.npz -l "..." --zrange 0,1000   (flux above 1000 m only)
    python -m nemoflux_amd.fluxplot -t T.nc -u U.nc -v V.nc -l "..." -s --tracer thetao --tracer-scale 4.1e-3
                                  (heat transport in PW: Sv degC x 1e6 m^3/s x rho0 c_p (4.1e6 J/m^3/K) x 1e-15 PW/W)
    python -m nemoflux_amd.fluxplot -t T.nc -u U.nc -v V.nc -l "..." -s --tracer sigma0 --tracer-file S.nc --classes 26,27,28
                                  (water flow by sigma0 class: one CSV line per time step and class)
    ... --tracer sigma0 --tracer-file S.nc --classes 26,27,28 --carry thetao --carry-scale 4.1e-3   (heat by sigma0 class)
    ... --sigma thetao,so[,PREF] --classes 26,27,28   (the same by sigma_PREF computed from thetao and so on the GPU: EOS-80,
                                  PREF in dbar, default 0; in place of --tracer for --classes, --gross-classes, --carry, --classes2)
    ... --sigma thetao,so --classes 26,26.01,...,28 --remap linear [--carry thetao]
                                  (conservative remapping: every level's transport spread over the classes between the class
                                  field's values at the layer's two interfaces -- a smooth MOC(sigma) with many class edges)
    ... --depth-bins 0,100,500,1000,6000 [--depth-top 0] [--tracer thetao] [--cell-thickness]
                                  (water flow, or the transport of thetao, in true-depth bins: a level's transport is spread over
                                  the bins its layer covers at each face -- with --cell-thickness the depths are sums of e3u / e3v)
    ... --depth-surfaces mldr10_1,iso20 [--surface-file S.nc] [--depth-top 0] [--tracer thetao] [--cell-thickness]
                                  (water flow, or the transport of thetao, in the layers bounded by 2-D fields: above the first
                                  surface, between consecutive ones, below the last; a layer that a surface cuts is split)
    ... --iso-depth 20 --iso-of thetao | --iso-depth 27.7,27.9 --sigma thetao,so [--iso-relative ZREF] [--iso-e3t e3t]
                                  (the same layers bounded by surfaces computed on the GPU: the depth at which a variable, or
                                  sigma_PREF of two, first reaches each value going down the column; --iso-sense rising|falling)
    ... --mixed-layer thetao,so[,DELTA[,ZREF]]   (above and below the mixed-layer depth: sigma0 exceeds its value at ZREF by DELTA)
    ... --levels [--tracer thetao]               (water flow, or the transport of thetao, of every level: one line per level)
    ... --tracer thetao --decompose              (the transport of thetao and its throughflow, overturning and gyre parts)
    ... --tracer thetao --eddy                   (the time-mean transport of thetao, its mean-flow part and its eddy part)
    ... --tracer thetao --eddy --cell-thickness --thickness-weighted   (the same for z* output: thickness-weighted mean flow)
    ... --tracer thetao --eddy --time-weights bounds --time-select months:12,1,2   (the DJF mean, months weighted by their length)
    ... --gross [--tracer thetao] [--zrange 0,700] (inflow, outflow and net of every transect; what they carry, their mean thetao)
    ... --tracer sigma0 --tracer-file S.nc --gross-classes 26,27,28 [--carry thetao] [--cell-thickness]
                                  (inflow, outflow and net of every sigma0 class: one CSV line per time step, transect and class)
    ... --sigma thetao,so --gross-classes 26,26.01,...,28 --gross-remap linear [--carry thetao] [--cell-thickness]
                                  (the same table by conservative remapping: smooth in the class, under e3u / e3v too)
    ... --tracer sigma0 --tracer-file S.nc --class-area 26,27,28 [--carry thetao] [--cell-thickness]
                                  (section area, mean carried tracer and interface depth of every sigma0 class: one CSV line
                                  per time step, transect and class; --sigma thetao,so in place of --tracer works too)
    ... --cell-thickness [--e3u NAME] [--e3v NAME] [--e3-file-u FILE] [--e3-file-v FILE]
                                  (partial steps / z*: the layer thicknesses e3u, e3v of the U and V files instead of deptht_bounds)
    ... --cell-thickness --e3t thkcello [--e3t-file FILE] [--e3-rule min|mean|anomaly] [--e3-static MESH[:E3T0,E3U0,E3V0]]
                                  (the same from the thickness at T points alone: e3u, e3v derived on the GPU step by step)
    ... --cell-thickness --ssh zos [--ssh-file FILE] --e3-static MESH[:E3U0,E3V0] [--e3-areas E1E2T,E1E2U,E1E2V]
                                  (z* output without a 3-D thickness: e3u, e3v from the sea surface height and the mesh file)
"""
import argparse
import glob
import os

import numpy

from . import _expr
from .field import Field
from .latlonreader import LatLonReader


def readTargets(lonLatPoints='', iFiles=''):
    """fluxplot.py:27-46: a list of polylines from a Python-list string or from station files."""
    names = []
    if lonLatPoints:
        pts = _expr.literal(lonLatPoints, 'lonLatPoints')
        if len(pts) and not isinstance(pts[0][0], (list, tuple)):
            pts = [pts]  # README.md:32 passes a single polyline without the outer list
        lonLatZPoints = [numpy.array([(ll[0], ll[1], 0.0) for ll in llp]) for llp in pts]
        names = [f'line{i}' for i in range(len(lonLatZPoints))]
    elif iFiles:
        try:      # fluxplot.py:37 evaluates a Python list of names; a glob pattern or a single name is accepted too
            listOfFiles = _expr.literal(iFiles, 'iFiles')
            if isinstance(listOfFiles, str):
                listOfFiles = [listOfFiles]
        except RuntimeError:
            listOfFiles = sorted(glob.glob(iFiles)) or [iFiles]
        lonLatZPoints = []
        for iFile in listOfFiles:
            ll = LatLonReader(iFile).getLonLats()
            lonLatZPoints.append(numpy.array([(p[0], p[1], 0.) for p in ll]))
            names.append(os.path.basename(iFile))
    else:
        raise RuntimeError('ERROR must provide either iFiles (-i) or lonLatPoints (-l)!')  # fluxplot.py:48
    return lonLatZPoints, names


def _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness=None):
    """the Field of a series: only totals are wanted, so no read-back, and only the signed edge fluxes stay resident (compact
    mode); cellThickness: ((path, name) of e3u, (path, name) of e3v) for Field.setCellThickness, or None"""
    fld = Field(tFile, uFile, vFile, lonLatZPoints, sverdrup, readback=False, compact=True)
    if cellThickness is not None:
        fld.setCellThickness(*cellThickness)
    return fld


def fluxSeries(tFile, uFile, vFile, lonLatZPoints, sverdrup=False, cellThickness=None):
    """(nt, ntransect) total fluxes and the Field (one batched GPU pass over every time step)."""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    totals, _ = fld.computeAll()
    return totals, fld


def bandSeries(tFile, uFile, vFile, lonLatZPoints, ztop, zbot, sverdrup=False, cellThickness=None):
    """(nt, ntransect) fluxes inside the depth band [ztop, zbot] and the Field: one depth-resolved step per time step."""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    totals = numpy.array([fld.depthBandFlux(fld.computeFluxProfile(t, prefetch_next=True)[0], ztop, zbot)
                          for t in range(fld.nt)]).reshape(fld.nt, len(lonLatZPoints))
    return totals, fld


def tracerSeries(tFile, uFile, vFile, lonLatZPoints, tracer, tracerFile='', tracerRef=0.0, sverdrup=False, cellThickness=None):
    """(nt, ntransect) tracer transports (Field.computeTracerAll) of the variable `tracer` of tracerFile (default: the T
    file) and the Field."""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    fld.setTracer((tracerFile or tFile, tracer), reference=tracerRef)
    totals, _ = fld.computeTracerAll()
    return totals, fld


def parseSigma(sigma):
    """'THETA,SALT[,PREF]' -> (theta name, salt name, pref in dbar): the variables of --sigma and its reference pressure"""
    parts = [x.strip() for x in sigma.split(',')]
    if len(parts) not in (2, 3) or not parts[0] or not parts[1]:
        raise RuntimeError(f'ERROR: --sigma must be THETA,SALT[,PREF] (two variable names and a pressure in dbar), got {sigma!r}')
    try:
        pref = float(parts[2]) if len(parts) == 3 else 0.0
    except ValueError:
        raise RuntimeError(f'ERROR: --sigma must be THETA,SALT[,PREF] with a number PREF, got {sigma!r}')
    if not (pref >= 0.0 and numpy.isfinite(pref)):
        raise RuntimeError(f'ERROR: --sigma needs a finite PREF >= 0 (dbar), got {sigma!r}')
    return parts[0], parts[1], pref


def sigmaName(pref):
    """what the tables call the class field of --sigma: sigma0, sigma2, sigma4 (PREF in 1000 dbar)"""
    return f'sigma{pref / 1000.0:g}'


def _classField(tFile, tracer, tracerFile, sigma):
    """the class field for setTracer / setClassTracer: the variable `tracer` of tracerFile (default: the T file), or with
    sigma = (theta name, salt name, pref) the potential density of those two variables of that file"""
    path = tracerFile or tFile
    if sigma is None:
        return (path, tracer)
    from .eos import Sigma
    return Sigma((path, sigma[0]), (path, sigma[1]), pref=sigma[2])


def classSeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, tracerFile='', sverdrup=False, sigma=None):
    """(nt, nedges+2, ntransect) water flow by class of the variable `tracer` of tracerFile (default: the T file; sigma: see
    _classField), one Field.computeClassTransport per time step, and the Field."""
    fld = Field(tFile, uFile, vFile, lonLatZPoints, sverdrup, readback=False, compact=True)
    fld.setTracer(_classField(tFile, tracer, tracerFile, sigma))
    fld.setClassEdges(edges)
    totals = numpy.array([fld.computeClassTransport(t, prefetch_next=True)[0] for t in range(fld.nt)])
    return totals.reshape(fld.nt, len(edges) + 2, len(lonLatZPoints)), fld


def carrySeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, carry, tracerFile='', carryFile='', carryRef=0.0,
                sverdrup=False, sigma=None):
    """(nt, nedges+2, ntransect) transport of the variable `carry` of carryFile by class of the variable `tracer` of
    tracerFile (default for both: the T file), one Field.computeClassTracerTransport per time step, and the Field."""
    fld = Field(tFile, uFile, vFile, lonLatZPoints, sverdrup, readback=False, compact=True)
    fld.setTracer((carryFile or tFile, carry), reference=carryRef)
    fld.setClassTracer(_classField(tFile, tracer, tracerFile, sigma))
    fld.setClassEdges(edges)
    totals = numpy.array([fld.computeClassTracerTransport(t, prefetch_next=True)[0] for t in range(fld.nt)])
    return totals.reshape(fld.nt, len(edges) + 2, len(lonLatZPoints)), fld


def remapSeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, carry='', tracerFile='', carryFile='', carryRef=0.0,
                sverdrup=False, sigma=None):
    """(nt, nedges+2, ntransect) rows of classSeries -- or, with `carry`, of carrySeries -- by conservative remapping, one
    Field.computeClassRemap per time step, and the Field."""
    fld = Field(tFile, uFile, vFile, lonLatZPoints, sverdrup, readback=False, compact=True)
    if carry:
        fld.setTracer((carryFile or tFile, carry), reference=carryRef)
        fld.setClassTracer(_classField(tFile, tracer, tracerFile, sigma))
    else:
        fld.setTracer(_classField(tFile, tracer, tracerFile, sigma))
    fld.setClassEdges(edges)
    totals = numpy.array([fld.computeClassRemap(t, carry=bool(carry), prefetch_next=True)[0] for t in range(fld.nt)])
    return totals.reshape(fld.nt, len(edges) + 2, len(lonLatZPoints)), fld


def jointClassSeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, tracer2, edges2, tracerFile='', tracer2File='',
                     sverdrup=False, sigma=None):
    """(nt, nA+2, nB+2, ntransect) water flow in joint classes of the variable `tracer` of tracerFile (edges) and the variable
    `tracer2` of tracer2File (edges2; default for both files: the T file), one Field.computeJointClassTransport per time
    step, and the Field."""
    fld = Field(tFile, uFile, vFile, lonLatZPoints, sverdrup, readback=False, compact=True)
    fld.setTracer(_classField(tFile, tracer, tracerFile, sigma))
    fld.setClassTracer((tracer2File or tFile, tracer2))
    fld.setJointClassEdges(edges, edges2)
    totals = numpy.array([fld.computeJointClassTransport(t, prefetch_next=True)[0] for t in range(fld.nt)])
    return totals.reshape(fld.nt, len(edges) + 2, len(edges2) + 2, len(lonLatZPoints)), fld


def levelSeries(tFile, uFile, vFile, lonLatZPoints, tracer='', tracerFile='', tracerRef=0.0, sverdrup=False, cellThickness=None):
    """(nt, nz, ntransect) water flow of every level (Field.computeFluxProfile) or, with `tracer`, the transport of that
    variable of tracerFile (default: the T file) of every level (Field.computeTracerProfile), and the Field."""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    if tracer:
        fld.setTracer((tracerFile or tFile, tracer), reference=tracerRef)
    profile = fld.computeTracerProfile if tracer else fld.computeFluxProfile
    totals = numpy.array([profile(t, prefetch_next=True)[0] for t in range(fld.nt)])
    return totals.reshape(fld.nt, fld.nz, len(lonLatZPoints)), fld


PARTS = ('total', 'throughflow', 'overturning', 'gyre')


def decomposeSeries(tFile, uFile, vFile, lonLatZPoints, tracer, tracerFile='', tracerRef=0.0, sverdrup=False, cellThickness=None):
    """(nt, 4, ntransect) transport of the variable `tracer` of tracerFile (default: the T file) and its throughflow,
    overturning and gyre parts (PARTS; Field.decomposeTracerTransport per time step), and the Field."""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    fld.setTracer((tracerFile or tFile, tracer), reference=tracerRef)
    totals = numpy.zeros((fld.nt, len(PARTS), len(lonLatZPoints)))
    for t in range(fld.nt):
        d = fld.decomposeTracerTransport(t)
        totals[t] = [d[k] for k in PARTS]
    return totals, fld


EDDY_PARTS = ('total', 'mean', 'eddy')


def parseTimeWeights(text):
    """--time-weights: 'bounds' (the step lengths of the file's time bounds) or W0,W1,... (one positive number per visited step)"""
    if text.strip() == 'bounds':
        return 'bounds'
    try:
        w = [float(x) for x in text.split(',')]
    except ValueError:
        raise RuntimeError(f"ERROR: --time-weights must be 'bounds' or W0,W1,... (numbers), got '{text}'")
    if not w or not all(x > 0 and x < numpy.inf for x in w):
        raise RuntimeError(f'ERROR: --time-weights: every weight must be finite and > 0, got {text}')
    return w


def parseTimeSelect(text):
    """--time-select: I0,I1,... (strictly ascending step indices) as a list, or months:M1,M2,... as ('months', [M1, ...])"""
    months = text.strip().startswith('months:')
    try:
        v = [int(x) for x in text.strip()[len('months:') if months else 0:].split(',')]
    except ValueError:
        raise RuntimeError(f"ERROR: --time-select must be I0,I1,... or months:M1,M2,... (whole numbers), got '{text}'")
    if months:
        if not all(1 <= m <= 12 for m in v):
            raise RuntimeError(f'ERROR: --time-select months:M1,M2,...: months are 1 to 12, got {text}')
        return ('months', v)
    if v[0] < 0 or any(b <= a for a, b in zip(v, v[1:])):
        raise RuntimeError(f'ERROR: --time-select I0,I1,...: step indices must be >= 0 and strictly ascending, got {text}')
    return v


def selectSteps(fld, timeSelect):
    """the step indices of a parsed --time-select on a Field: the list itself, or the steps whose month is one of the months"""
    if not timeSelect or timeSelect[0] != 'months':
        return timeSelect or None
    months = getattr(fld.timeObj, 'getMonths', lambda: None)()
    if not months or any(m is None for m in months):
        raise RuntimeError('ERROR: --time-select months:... needs a time variable with decodable units in the U file')
    steps = [t for t, m in enumerate(months) if m in timeSelect[1]]
    if not steps:
        raise RuntimeError(f'ERROR: --time-select months:{",".join(str(m) for m in timeSelect[1])} selects no time step')
    return steps


def eddySeries(tFile, uFile, vFile, lonLatZPoints, tracer, tracerFile='', tracerRef=0.0, sverdrup=False, cellThickness=None,
               thicknessWeighted=False, timeWeights=None, timeSelect=None):
    """(3, ntransect): the mean over all time steps of the transport of the variable `tracer` of tracerFile (default: the T
    file), the transport of the time-mean tracer by the time-mean flow, and their difference, the eddy part (EDDY_PARTS;
    Field.meanEddyTracerTransport), and the Field.  thicknessWeighted: the mean flow of a time-varying cell thickness, the
    mean thickness times the thickness-weighted mean velocity.  timeWeights / timeSelect (parseTimeWeights, parseTimeSelect):
    the weights and the selection of the steps of the mean; the Field keeps the selected steps in _eddy_steps."""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    fld.setTracer((tracerFile or tFile, tracer), reference=tracerRef)
    if timeWeights or timeSelect:
        fld._eddy_steps = selectSteps(fld, timeSelect)
        d = fld.meanEddyTracerTransport(thicknessWeighted=thicknessWeighted, select=fld._eddy_steps, weights=timeWeights or None)
    else:
        d = fld.meanEddyTracerTransport(thicknessWeighted=thicknessWeighted)
    return numpy.array([d[k] for k in EDDY_PARTS]).reshape(len(EDDY_PARTS), len(lonLatZPoints)), fld


GROSS_COLUMNS = ('inflow', 'outflow', 'net')
GROSS_TRACER_COLUMNS = ('carried_in', 'carried_out', 'mean_in', 'mean_out')


def grossSeries(tFile, uFile, vFile, lonLatZPoints, tracer='', tracerFile='', tracerRef=0.0, tracerScale=1.0, zrange=None,
                sverdrup=False, cellThickness=None):
    """(nt, ntransect, 3) inflow, outflow and net water flow of every transect (GROSS_COLUMNS: Field.computeGrossProfile, summed
    over the depth or the band zrange = (ztop, zbot) by Field.grossTransport; net = inflow + outflow) and the Field.  With
    `tracer` (nt, ntransect, 7): also what the inflow and the outflow carry of that variable of tracerFile (default: the T
    file), times tracerScale, and the transport-weighted mean tracer of each (GROSS_TRACER_COLUMNS;
    Field.transportWeightedTracer, NaN where nothing flows that way)."""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    if tracer:
        fld.setTracer((tracerFile or tFile, tracer), reference=tracerRef)
    band = dict(ztop=zrange[0], zbot=zrange[1], bounds_depth=fld.bounds_depth) if zrange else {}
    totals = numpy.zeros((fld.nt, len(lonLatZPoints), 7 if tracer else 3))
    for t in range(fld.nt):
        vol = fld.grossTransport(fld.computeGrossProfile(t, prefetch_next=not tracer)[0], **band)
        totals[t, :, 0], totals[t, :, 1], totals[t, :, 2] = vol[0], vol[1], vol[0] + vol[1]
        if tracer:
            car = fld.grossTransport(fld.computeGrossProfile(t, carry=True, prefetch_next=True)[0], **band)
            mean = fld.transportWeightedTracer(vol, car, tracerRef)
            totals[t, :, 3], totals[t, :, 4] = car[0] * float(tracerScale), car[1] * float(tracerScale)
            totals[t, :, 5], totals[t, :, 6] = mean[0], mean[1]
    return totals, fld


def grossClassSeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, tracerFile='', carry='', carryFile='', carryRef=0.0,
                     sverdrup=False, cellThickness=None, sigma=None, remap=False):
    """(nt, 2, nedges+2, ntransect) inflow and outflow of every class of the variable `tracer` of tracerFile (default: the T
    file), one Field.computeGrossClassTransport per time step, and the Field.  With `carry`: what they carry of that variable
    of carryFile (reference carryRef) instead of the water.  remap: one Field.computeGrossClassRemap per step instead."""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    if carry:
        fld.setTracer((carryFile or tFile, carry), reference=carryRef)
        fld.setClassTracer(_classField(tFile, tracer, tracerFile, sigma))
    else:
        fld.setTracer(_classField(tFile, tracer, tracerFile, sigma))
    fld.setClassEdges(edges)
    step = fld.computeGrossClassRemap if remap else fld.computeGrossClassTransport
    totals = numpy.array([step(t, carry=bool(carry), prefetch_next=True)[0] for t in range(fld.nt)])
    return totals.reshape(fld.nt, 2, len(edges) + 2, len(lonLatZPoints)), fld


def grossRemapSeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, tracerFile='', carry='', carryFile='', carryRef=0.0,
                     sverdrup=False, cellThickness=None, sigma=None):
    """(nt, 2, nedges+2, ntransect) rows of grossClassSeries by conservative remapping, one Field.computeGrossClassRemap per time
    step, and the Field: what remapSeries is to classSeries, and with cellThickness the one remapped table under e3u / e3v."""
    return grossClassSeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, tracerFile, carry, carryFile, carryRef, sverdrup,
                            cellThickness, sigma, remap=True)


def checkGrossRemapArgs(grossRemap='', grossClasses='', classes=''):
    """the --gross-remap option of the command line (conservative remapping of the table of --gross-classes): refused
    combinations raise RuntimeError"""
    if not grossRemap:
        return
    if grossRemap != 'linear':
        raise RuntimeError(f"ERROR: --gross-remap must be 'linear' (piecewise-linear conservative remapping), got {grossRemap!r}")
    if classes:
        raise RuntimeError('ERROR: --gross-remap and --classes cannot be combined: --gross-remap applies to the table of '
                           '--gross-classes (--remap is the option of --classes)')
    if not grossClasses:
        raise RuntimeError('ERROR: --gross-remap needs --gross-classes E0,...,EN (with --tracer NAME or --sigma THETA,SALT[,PREF]; '
                           '--carry NAME and --cell-thickness apply)')


def checkGrossClassArgs(grossClasses='', tracer='', tracerRef=0.0, tracerScale=1.0, classes='', classes2='', gross=False,
                        levels=False, zrange='', decompose=False, eddy=False, show=False):
    """the --gross-classes option of the command line (inflow and outflow of every tracer class): refused combinations raise
    RuntimeError"""
    if not grossClasses:
        return
    if not tracer:
        raise RuntimeError('ERROR: --gross-classes needs --tracer NAME (the class field, e.g. sigma0 or thetao)')
    for on, opt in ((classes, '--classes'), (classes2, '--classes2'), (gross, '--gross'), (levels, '--levels'),
                    (zrange, '--zrange'), (decompose, '--decompose'), (eddy, '--eddy'), (show, '--show')):
        if on:
            raise RuntimeError(f'ERROR: --gross-classes and {opt} cannot be combined: --gross-classes writes the inflow, the '
                               f'outflow and the net transport of every class of --tracer (with --carry NAME: of NAME) as CSV '
                               f'only')
    if float(tracerRef) != 0.0 or float(tracerScale) != 1.0:
        raise RuntimeError('ERROR: --gross-classes bins by the raw tracer: --tracer-ref / --tracer-scale do not apply '
                           '(--carry-ref / --carry-scale do, with --carry NAME)')
    try:
        parseClasses(grossClasses)
    except RuntimeError as e:
        raise RuntimeError(str(e).replace('--classes', '--gross-classes'))


CLASS_AREA_COLUMNS = ('area', 'mean', 'depth')


def classAreaSeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, tracerFile='', carry='', carryFile='', carryRef=0.0,
                    cellThickness=None, sigma=None):
    """(nt, 3, nedges+2, ntransect), CLASS_AREA_COLUMNS: the section area that every class of the variable `tracer` of
    tracerFile (default: the T file) occupies, the area-weighted mean of the carried tracer in it -- `carry` of carryFile
    (reference carryRef), else the class field itself -- and the pseudo-depth of the class's upper edge (NaN for the two last
    rows, which have none), and the Field: Field.computeClassArea and Field.computeAreaProfile per time step, then
    Field.classMeanTracer and Field.classInterfaceDepth on the transect totals."""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, False, cellThickness)
    if carry:
        fld.setTracer((carryFile or tFile, carry), reference=carryRef)
        fld.setClassTracer(_classField(tFile, tracer, tracerFile, sigma))
    else:
        fld.setTracer(_classField(tFile, tracer, tracerFile, sigma))
    fld.setClassEdges(edges)
    totals = numpy.full((fld.nt, 3, len(edges) + 2, len(lonLatZPoints)), numpy.nan)
    for t in range(fld.nt):
        parts = fld.computeClassArea(t)[0]
        byLevel = fld.computeAreaProfile(t, prefetch_next=True)[0][0]
        totals[t, 0] = parts[0]
        totals[t, 1] = fld.classMeanTracer(parts, carryRef if carry else 0.0)
        totals[t, 2, :len(edges)] = fld.classInterfaceDepth(parts[0], byLevel, fld.bounds_depth)
    return totals, fld


def checkClassAreaArgs(classArea='', tracer='', tracerRef=0.0, tracerScale=1.0, carryScale=1.0, classes='', classes2='',
                       gross=False, grossClasses='', levels=False, zrange='', decompose=False, eddy=False, show=False):
    """the --class-area option of the command line (section area, mean tracer and interface depth of every tracer class):
    refused combinations raise RuntimeError"""
    if not classArea:
        return
    if not tracer:
        raise RuntimeError('ERROR: --class-area needs --tracer NAME or --sigma THETA,SALT[,PREF] (the class field, e.g. sigma0)')
    for on, opt in ((classes, '--classes'), (classes2, '--classes2'), (gross, '--gross'), (grossClasses, '--gross-classes'),
                    (levels, '--levels'), (zrange, '--zrange'), (decompose, '--decompose'), (eddy, '--eddy'), (show, '--show')):
        if on:
            raise RuntimeError(f'ERROR: --class-area and {opt} cannot be combined: --class-area writes the section area, the mean '
                               f'carried tracer and the interface depth of every class of --tracer as CSV only')
    if float(tracerRef) != 0.0 or float(tracerScale) != 1.0:
        raise RuntimeError('ERROR: --class-area bins by the raw tracer: --tracer-ref / --tracer-scale do not apply '
                           '(--carry-ref does, with --carry NAME)')
    if float(carryScale) != 1.0:
        raise RuntimeError('ERROR: --class-area writes the mean of --carry NAME, not a transport: --carry-scale does not apply')
    try:
        parseClasses(classArea)
    except RuntimeError as e:
        raise RuntimeError(str(e).replace('--classes', '--class-area'))


CROSSINGS_MAX_BYTES = 2 << 30


def crossingsSeries(tFile, uFile, vFile, lonLatZPoints, path, tracer='', tracerFile='', tracerRef=0.0, zrange=None,
                    sverdrup=False, cellThickness=None, sigma=None):
    """--crossings FILE.npz: for every time step the planes of Field.computeCrossings -- (nt, 2, nz, ncross) = q, g, or with a
    tracer (a variable, or sigma = (theta, salt, pref)) (nt, 4, nz, ncross) = q, c, a, b -- the cumulative transport along
    every transect (nt, ncross), over the depth or the band zrange = (ztop, zbot), and the arrays of Field.getCrossings(),
    written to `path` with numpy.savez.  Returns (planes, cumulative, Field).  Refused when the planes would exceed 2 GiB: the
    file is for sections, not for batches of basin-wide transects."""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    carried = bool(tracer) or sigma is not None
    if carried:
        fld.setTracer(_classField(tFile, tracer, tracerFile, sigma), reference=tracerRef)
    cr = fld.getCrossings()
    nplanes = 4 if carried else 2
    nbytes = 8 * fld.nt * nplanes * fld.nz * len(cr)
    if nbytes > CROSSINGS_MAX_BYTES:
        raise RuntimeError(f'ERROR: --crossings would write {nbytes / 2.**30:.1f} GiB ({fld.nt} steps x {nplanes} planes x {fld.nz} '
                           f'levels x {len(cr)} crossings x 8 bytes), more than 2 GiB: it is meant for sections -- give fewer or '
                           f'shorter transects')
    planes = numpy.zeros((fld.nt, nplanes, fld.nz, len(cr)))
    cumulative = numpy.zeros((fld.nt, len(cr)))
    band = dict(ztop=zrange[0], zbot=zrange[1], bounds_depth=fld.bounds_depth) if zrange else {}
    for t in range(fld.nt):
        planes[t] = fld.computeCrossings(t, carry=carried, prefetch_next=True)
        cumulative[t] = fld.cumulativeTransport(planes[t], cr, **band)
    numpy.savez(path, planes=planes, plane_names=numpy.array(['q', 'c', 'a', 'b'] if carried else ['q', 'g']),
                cumulative=cumulative, bounds_depth=numpy.asarray(fld.bounds_depth), reference=float(tracerRef),
                sverdrup=bool(sverdrup), **cr.asdict())
    return planes, cumulative, fld


def checkCrossingsArgs(crossings='', **others):
    """the --crossings option of the command line: it writes its own file and combines with --tracer / --sigma, --tracer-ref,
    --zrange, --cell-thickness and -s alone; refused combinations raise RuntimeError"""
    if not crossings:
        return
    for opt, on in others.items():
        if on:
            raise RuntimeError(f'ERROR: --crossings and {opt} cannot be combined: --crossings writes the per-crossing planes of '
                               f'every time step to its own file')


def depthSeries(tFile, uFile, vFile, lonLatZPoints, edges, top=0.0, tracer='', tracerFile='', tracerRef=0.0, sverdrup=False,
                cellThickness=None):
    """(nt, nedges+2, ntransect) water flow -- or, with `tracer`, transport of that variable of tracerFile (default: the T
    file) -- in the true-depth bins of `edges`, one Field.computeDepthTransport per time step, and the Field.  With
    cellThickness the depth of a layer is the running sum of the cell thicknesses at its own face."""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    if tracer:
        fld.setTracer((tracerFile or tFile, tracer), reference=tracerRef)
    fld.setDepthEdges(edges, top)
    totals = numpy.array([fld.computeDepthTransport(t, carry=bool(tracer), prefetch_next=True)[0] for t in range(fld.nt)])
    return totals.reshape(fld.nt, len(edges) + 2, len(lonLatZPoints)), fld


def checkDepthBinsArgs(depthBins='', depthTop=0.0, **others):
    """the --depth-bins option of the command line (transports in true-depth bins): it combines with --depth-top, --tracer
    (with --tracer-file, --tracer-ref, --tracer-scale), --cell-thickness and -s alone; refused combinations raise
    RuntimeError"""
    if not depthBins:
        if float(depthTop) != 0.0:
            raise RuntimeError('ERROR: --depth-top needs --depth-bins E0,...,EN')
        return
    for opt, on in others.items():
        if on:
            raise RuntimeError(f'ERROR: --depth-bins and {opt} cannot be combined: --depth-bins writes the transport in every '
                               f'depth bin as CSV only')
    if not numpy.isfinite(float(depthTop)):
        raise RuntimeError(f'ERROR: --depth-top must be a finite number, got {depthTop!r}')
    try:
        parseClasses(depthBins)
    except RuntimeError as e:
        raise RuntimeError(str(e).replace('--classes', '--depth-bins'))


def surfaceSeries(tFile, uFile, vFile, lonLatZPoints, names, surfaceFile='', top=0.0, tracer='', tracerFile='', tracerRef=0.0,
                  sverdrup=False, cellThickness=None):
    """(nt, m+2, ntransect) water flow -- or, with `tracer`, transport of that variable of tracerFile (default: the T file) --
    in the layers bounded by the 2-D variables `names` of surfaceFile (default: the T file), one
    Field.computeSurfaceTransport per time step, and the Field"""
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    if tracer:
        fld.setTracer((tracerFile or tFile, tracer), reference=tracerRef)
    fld.setDepthSurfaces([(surfaceFile or tFile, n) for n in names], top=top)
    totals = numpy.array([fld.computeSurfaceTransport(t, carry=bool(tracer), prefetch_next=True)[0] for t in range(fld.nt)])
    return totals.reshape(fld.nt, len(names) + 2, len(lonLatZPoints)), fld


def parseSurfaces(text):
    """--depth-surfaces: NAME[,NAME...], 1 to 8 variable names"""
    names = [x.strip() for x in text.split(',')]
    if not 1 <= len(names) <= 8 or not all(names):
        raise RuntimeError(f"ERROR: --depth-surfaces must be NAME[,NAME...] with 1 to 8 variable names, got '{text}'")
    return names


def checkDepthSurfacesArgs(depthSurfaces='', surfaceFile='', depthTop=0.0, **others):
    """the --depth-surfaces option of the command line (transports between surfaces): it combines with --surface-file,
    --depth-top, --tracer (with --tracer-file, --tracer-ref, --tracer-scale), --cell-thickness and -s alone; refused
    combinations raise RuntimeError"""
    if not depthSurfaces:
        if surfaceFile:
            raise RuntimeError('ERROR: --surface-file needs --depth-surfaces NAME[,NAME...]')
        return
    for opt, on in others.items():
        if on:
            raise RuntimeError(f'ERROR: --depth-surfaces and {opt} cannot be combined: --depth-surfaces writes the transport in '
                               f'every layer between the surfaces as CSV only')
    if not numpy.isfinite(float(depthTop)):
        raise RuntimeError(f'ERROR: --depth-top must be a finite number, got {depthTop!r}')
    parseSurfaces(depthSurfaces)


def parseIsoValues(text):
    """--iso-depth: V1[,...,Vm], 1 to 8 finite numbers"""
    try:
        v = [float(x) for x in text.split(',')]
    except ValueError:
        raise RuntimeError(f"ERROR: --iso-depth must be V1[,...,Vm] (numbers), got '{text}'")
    if not 1 <= len(v) <= 8 or not all(numpy.isfinite(v)):
        raise RuntimeError(f"ERROR: --iso-depth needs 1 to 8 finite values (one surface each), got '{text}'")
    return v


def parseMixedLayer(text):
    """--mixed-layer: 'THETA,SALT[,DELTA[,ZREF]]' -> (theta name, salt name, delta in kg m-3, zref); defaults 0.03 and 10"""
    parts = [x.strip() for x in text.split(',')]
    if len(parts) not in (2, 3, 4) or not parts[0] or not parts[1]:
        raise RuntimeError(f"ERROR: --mixed-layer must be THETA,SALT[,DELTA[,ZREF]] (two variable names, a density step and a "
                           f"reference depth), got '{text}'")
    try:
        delta = float(parts[2]) if len(parts) > 2 else 0.03
        zref = float(parts[3]) if len(parts) > 3 else 10.0
    except ValueError:
        raise RuntimeError(f"ERROR: --mixed-layer must be THETA,SALT[,DELTA[,ZREF]] with numbers DELTA and ZREF, got '{text}'")
    if not (numpy.isfinite(delta) and numpy.isfinite(zref)):
        raise RuntimeError(f"ERROR: --mixed-layer needs finite DELTA and ZREF, got '{text}'")
    return parts[0], parts[1], delta, zref


def checkIsoDepthArgs(isoDepth='', isoOf='', isoSense='', isoRelative='', isoE3t='', mixedLayer='', sigma='', depthSurfaces='',
                      depthTop=0.0, **others):
    """the --iso-depth and --mixed-layer options of the command line (transports between surfaces computed on the GPU): they
    combine with --surface-file, --depth-top, --tracer (with --tracer-file, --tracer-ref, --tracer-scale), --cell-thickness
    and -s as --depth-surfaces does; refused combinations raise RuntimeError.  Returns what isoSurfaceSeries takes, or None."""
    if not (isoDepth or mixedLayer):
        for on, opt in ((isoOf, '--iso-of'), (isoSense, '--iso-sense'), (isoRelative != '', '--iso-relative')):
            if on:
                raise RuntimeError(f'ERROR: {opt} needs --iso-depth V1[,...,Vm]')
        if isoE3t:
            raise RuntimeError('ERROR: --iso-e3t needs --iso-depth V1[,...,Vm] or --mixed-layer THETA,SALT')
        return None
    opt = '--iso-depth' if isoDepth else '--mixed-layer'
    if isoDepth and mixedLayer:
        raise RuntimeError('ERROR: --iso-depth and --mixed-layer cannot be combined: each writes the layers of its own surfaces')
    if depthSurfaces:
        raise RuntimeError(f'ERROR: {opt} and --depth-surfaces cannot be combined: the surfaces are either read (--depth-surfaces) '
                           f'or computed ({opt})')
    for name, on in others.items():
        if on:
            raise RuntimeError(f'ERROR: {opt} and {name} cannot be combined: {opt} writes the transport in every layer between '
                               f'the surfaces as CSV only')
    if not numpy.isfinite(float(depthTop)):
        raise RuntimeError(f'ERROR: --depth-top must be a finite number, got {depthTop!r}')
    if mixedLayer:
        for on, name in ((isoOf, '--iso-of'), (isoSense, '--iso-sense'), (isoRelative != '', '--iso-relative'), (sigma, '--sigma')):
            if on:
                raise RuntimeError(f'ERROR: --mixed-layer and {name} cannot be combined: --mixed-layer THETA,SALT[,DELTA[,ZREF]] '
                                   f'is the whole criterion')
        theta, salt, delta, zref = parseMixedLayer(mixedLayer)
        return dict(sigma=(theta, salt, 0.0), of='', values=[delta], sense=1, relative=True, zref=zref, e3t=isoE3t,
                    labels=['mld'])
    if bool(isoOf) == bool(sigma):
        raise RuntimeError('ERROR: --iso-depth needs exactly one of --iso-of NAME (the variable whose iso-surfaces are wanted) '
                           'and --sigma THETA,SALT[,PREF] (its potential density)')
    values = parseIsoValues(isoDepth)
    if isoSense and isoSense not in ('rising', 'falling'):
        raise RuntimeError(f"ERROR: --iso-sense must be 'rising' (the variable rises downward, as density does) or 'falling' (as "
                           f"temperature does), got '{isoSense}'")
    sense = {'rising': 1, 'falling': -1}[isoSense or ('rising' if sigma else 'falling')]
    relative, zref = isoRelative != '', 10.0
    if relative:
        try:
            zref = float(isoRelative)
        except ValueError:
            zref = numpy.nan
        if not numpy.isfinite(zref):
            raise RuntimeError(f"ERROR: --iso-relative must be ZREF, a finite depth, got '{isoRelative}'")
    sig = parseSigma(sigma) if sigma else None
    name = sigmaName(sig[2]) if sig else isoOf
    labels = [f'{name}@{zref:g}{v:+g}' if relative else f'{name}={v:g}' for v in values]
    return dict(sigma=sig, of=isoOf, values=values, sense=sense, relative=relative, zref=zref, e3t=isoE3t, labels=labels)


def isoSurfaceSeries(tFile, uFile, vFile, lonLatZPoints, spec, surfaceFile='', top=0.0, tracer='', tracerFile='', tracerRef=0.0,
                     sverdrup=False, cellThickness=None):
    """surfaceSeries with surfaces computed on the GPU (spec: checkIsoDepthArgs): (nt, m+2, ntransect) water flow -- or, with
    `tracer`, transport of that variable -- in the layers bounded by the depths at which a variable of surfaceFile (default:
    the T file), or the potential density of two, first reaches each value, one Field.computeSurfaceTransport per time step,
    and the Field"""
    from .surfaces import IsoDepth
    path = surfaceFile or tFile
    fld = _field(tFile, uFile, vFile, lonLatZPoints, sverdrup, cellThickness)
    if tracer:
        fld.setTracer((tracerFile or tFile, tracer), reference=tracerRef)
    source = _classField(path, spec['of'], '', spec['sigma'])
    item = IsoDepth(source, spec['values'], spec['sense'], e3t=(path, spec['e3t']) if spec['e3t'] else None,
                    relative=spec['relative'], zref=spec['zref'])
    fld.setDepthSurfaces([item], top=top)
    totals = numpy.array([fld.computeSurfaceTransport(t, carry=bool(tracer), prefetch_next=True)[0] for t in range(fld.nt)])
    return totals.reshape(fld.nt, item.m + 2, len(lonLatZPoints)), fld


def checkGrossArgs(gross=False, classes='', levels=False, decompose=False, eddy=False, show=False):
    """the --gross option of the command line: refused combinations raise RuntimeError"""
    if not gross:
        return
    for on, opt in ((classes, '--classes'), (levels, '--levels'), (decompose, '--decompose'), (eddy, '--eddy'), (show, '--show')):
        if on:
            raise RuntimeError(f'ERROR: --gross and {opt} cannot be combined: --gross writes the inflow, the outflow and the net '
                               f'transport of every transect (with --tracer what they carry, and their mean tracer) as CSV only')


def checkEddyArgs(eddy=False, tracer='', classes='', levels=False, zrange='', show=False, decompose=False):
    """the --eddy option of the command line: refused combinations raise RuntimeError"""
    if not eddy:
        return
    if not tracer:
        raise RuntimeError('ERROR: --eddy needs --tracer NAME (the tracer whose mean transport is split in time)')
    for on, opt in ((classes, '--classes'), (levels, '--levels'), (zrange, '--zrange'), (show, '--show'),
                    (decompose, '--decompose')):
        if on:
            raise RuntimeError(f'ERROR: --eddy and {opt} cannot be combined: --eddy writes the time-mean transport of --tracer, '
                               f'its mean-flow part and its eddy part as CSV only')


def checkThicknessWeightedArgs(thicknessWeighted=False, eddy=False, cellThickness=False):
    """the --thickness-weighted option of the command line: refused combinations raise RuntimeError"""
    if thicknessWeighted and not (eddy and cellThickness):
        raise RuntimeError('ERROR: --thickness-weighted needs --eddy and --cell-thickness: it splits the mean transport of '
                           '--tracer with the thickness-weighted mean flow of time-varying layer thicknesses (z*)')


def checkTimeMeanArgs(timeWeights='', timeSelect='', eddy=False):
    """the --time-weights and --time-select options of the command line: they weight and select the steps of the time mean of
    --eddy and are refused anywhere else; a value that does not parse raises RuntimeError too"""
    for on, opt in ((timeWeights, '--time-weights'), (timeSelect, '--time-select')):
        if on and not eddy:
            raise RuntimeError(f'ERROR: {opt} needs --eddy: it chooses the steps, or their weights, of the time mean that --eddy '
                               f'splits; no other table is a time mean')
    if timeWeights:
        parseTimeWeights(timeWeights)
    if timeSelect:
        parseTimeSelect(timeSelect)


def checkDecomposeArgs(decompose=False, tracer='', classes='', levels=False, zrange='', show=False):
    """the --decompose option of the command line: refused combinations raise RuntimeError"""
    if not decompose:
        return
    if not tracer:
        raise RuntimeError('ERROR: --decompose needs --tracer NAME (the tracer whose transport is split)')
    for on, opt in ((classes, '--classes'), (levels, '--levels'), (zrange, '--zrange'), (show, '--show')):
        if on:
            raise RuntimeError(f'ERROR: --decompose and {opt} cannot be combined: --decompose writes the total, throughflow, '
                               f'overturning and gyre parts of the full-depth transport of --tracer as CSV only')


def parseClasses(classes):
    """'E0,E1,...,EN' -> the class edges (a list of at least two finite, strictly increasing numbers)."""
    try:
        edges = [float(x) for x in classes.split(',')]
    except ValueError:
        raise RuntimeError(f'ERROR: --classes must be E0,E1,...,EN (numbers), got {classes!r}')
    if len(edges) < 2 or not all(numpy.isfinite(edges)) or not all(a < b for a, b in zip(edges, edges[1:])):
        raise RuntimeError(f'ERROR: --classes needs at least two finite, strictly increasing edges, got {classes!r}')
    return edges


def checkClassArgs(classes='', tracer='', tracerRef=0.0, tracerScale=1.0, zrange='', show=False):
    """the --classes option of the command line: refused combinations raise RuntimeError"""
    if not classes:
        return
    if not tracer:
        raise RuntimeError('ERROR: --classes needs --tracer NAME (the class field, e.g. sigma0 or thetao)')
    if zrange:
        raise RuntimeError('ERROR: --classes and --zrange cannot be combined: depth-resolved class transports are not '
                           'available')
    if float(tracerRef) != 0.0 or float(tracerScale) != 1.0:
        raise RuntimeError('ERROR: --classes bins the water flow by the raw tracer: --tracer-ref / --tracer-scale do not '
                           'apply')
    if show:
        raise RuntimeError('ERROR: --classes and --show cannot be combined: the class table is written as CSV only')
    parseClasses(classes)


def checkRemapArgs(remap='', classes='', tracer='', classes2='', levels=False, decompose=False, eddy=False):
    """the --remap option of the command line (conservative remapping of the class transport of --classes, with or without
    --carry): refused combinations raise RuntimeError"""
    if not remap:
        return
    if remap != 'linear':
        raise RuntimeError(f"ERROR: --remap must be 'linear' (piecewise-linear conservative remapping), got {remap!r}")
    if not (classes and tracer):
        raise RuntimeError('ERROR: --remap needs --classes E0,...,EN and --tracer NAME or --sigma THETA,SALT[,PREF] (the class '
                           'field): it spreads the class transport of --classes, or of --classes --carry NAME')
    for on, opt in ((classes2, '--classes2'), (levels, '--levels'), (decompose, '--decompose'), (eddy, '--eddy')):
        if on:
            raise RuntimeError(f'ERROR: --remap and {opt} cannot be combined: --remap applies to the table of --classes')


def checkJointClassArgs(classes2='', tracer2='', tracer2File='', tracer='', classes='', carry='', levels=False, zrange='',
                        show=False, eddy=False, decompose=False):
    """the --tracer2 / --classes2 options of the command line (the water flow in joint classes of two tracers): refused
    combinations raise RuntimeError"""
    if not classes2:
        if tracer2 or tracer2File:
            raise RuntimeError('ERROR: --tracer2 / --tracer2-file need --classes2 F0,...,FM (the class edges of the second '
                               'tracer)')
        return
    if not (tracer2 and tracer and classes):
        raise RuntimeError('ERROR: --classes2 needs --tracer2 NAME together with --tracer NAME and --classes E0,...,EN (the two '
                           'class fields and their edges)')
    for on, opt in ((carry, '--carry'), (levels, '--levels'), (zrange, '--zrange'), (show, '--show'), (eddy, '--eddy'),
                    (decompose, '--decompose')):
        if on:
            raise RuntimeError(f'ERROR: --classes2 and {opt} cannot be combined: --classes2 writes the water flow in joint '
                               f'classes of --tracer and --tracer2 as CSV only')
    try:
        edges2 = parseClasses(classes2)
    except RuntimeError as e:
        raise RuntimeError(str(e).replace('--classes', '--classes2'))
    n = (len(parseClasses(classes)) + 2) * (len(edges2) + 2)
    if n > 16384:
        raise RuntimeError(f'ERROR: --classes and --classes2 give {n} joint classes; at most 16384 are supported')


def checkCarryArgs(carry='', carryFile='', carryRef=0.0, carryScale=1.0, classes='', tracer='', levels=False):
    """the --carry options of the command line (the transport of a second tracer by class): refused combinations raise
    RuntimeError"""
    if not carry:
        if carryFile:
            raise RuntimeError('ERROR: --carry-file needs --carry NAME (the variable to read from it)')
        if float(carryRef) != 0.0 or float(carryScale) != 1.0:
            raise RuntimeError('ERROR: --carry-ref / --carry-scale need --carry NAME')
        return
    if levels:
        raise RuntimeError('ERROR: --carry and --levels cannot be combined: --levels --tracer NAME gives the transport of NAME '
                           'per level')
    if not classes or not tracer:
        raise RuntimeError('ERROR: --carry needs --classes E0,...,EN and --tracer NAME (the class field); the transport of a '
                           'tracer alone is --tracer NAME')
    for name, x in (('--carry-ref', carryRef), ('--carry-scale', carryScale)):
        if not numpy.isfinite(float(x)):
            raise RuntimeError(f'ERROR: {name} must be a finite number, got {x!r}')


def checkLevelsArgs(levels=False, zrange='', classes='', show=False):
    """the --levels option of the command line (one line per time step and level): refused combinations raise RuntimeError"""
    if not levels:
        return
    if zrange:
        raise RuntimeError('ERROR: --levels and --zrange cannot be combined: --levels lists every level, --zrange sums a band')
    if classes:
        raise RuntimeError('ERROR: --levels and --classes cannot be combined: depth-resolved class transports are not available')
    if show:
        raise RuntimeError('ERROR: --levels and --show cannot be combined: the level table is written as CSV only')


def checkCellThicknessArgs(cellThickness=False, e3u='', e3v='', e3FileU='', e3FileV='', classes='', carry='', levels=False,
                           tracer=''):
    """the --cell-thickness options of the command line: refused combinations raise RuntimeError"""
    if not cellThickness:
        if e3u or e3v or e3FileU or e3FileV:
            raise RuntimeError('ERROR: --e3u / --e3v / --e3-file-u / --e3-file-v need --cell-thickness')
        return
    if classes or carry:
        raise RuntimeError('ERROR: --cell-thickness cannot be combined with --classes / --carry: the class transports do not '
                           'take per-cell thicknesses yet')
    if levels and tracer:
        raise RuntimeError('ERROR: --cell-thickness cannot be combined with --levels --tracer: the tracer transport per level '
                           'does not take per-cell thicknesses yet (--levels alone, or --tracer alone, does)')


def checkSshArgs(cellThickness, ssh='', sshFile='', e3Areas='', e3Static='', e3t='', e3tFile='', e3u='', e3v='', e3FileU='',
                 e3FileV='', e3Rule=''):
    """the --ssh options of the command line: None without --ssh, else (the mesh file, the names of the two static thicknesses,
    the names of the three areas or None); refused combinations raise RuntimeError"""
    if not ssh:
        if sshFile or e3Areas:
            raise RuntimeError('ERROR: --ssh-file / --e3-areas need --ssh NAME (and --cell-thickness)')
        return None
    if e3t or e3tFile or e3u or e3v or e3FileU or e3FileV or e3Rule:
        raise RuntimeError('ERROR: --ssh cannot be combined with --e3t / --e3u / --e3v / --e3-rule: the thicknesses at the '
                           'U and V points are either read, derived from --e3t or derived from --ssh')
    if not cellThickness:
        raise RuntimeError('ERROR: --ssh needs --cell-thickness')
    if not e3Static:
        raise RuntimeError('ERROR: --ssh needs --e3-static MESH[:E3U0,E3V0], the mesh file that holds the static thicknesses '
                           'at the U and V points')
    path, sep, tail = e3Static.rpartition(':')
    # a tail without a path separator is a list of names (one name is an error, not a file called MESH:NAME)
    if sep and path and '/' not in tail and '\\' not in tail:
        names = tail.split(',')
        if len(names) != 2 or not all(names):
            raise RuntimeError(f'ERROR: with --ssh, --e3-static must be MESH or MESH:E3U0,E3V0 (two names), got {e3Static!r}')
    else:
        path, names = e3Static, ['e3u_0', 'e3v_0']
    anames = None
    if e3Areas:
        anames = e3Areas.split(',')
        if len(anames) != 3 or not all(anames):
            raise RuntimeError(f'ERROR: --e3-areas must be E1E2T,E1E2U,E1E2V (three names of the mesh file), got {e3Areas!r}')
    return path, names, anames


def cellThicknessSource(cellThickness, tFile, uFile, vFile, e3u='', e3v='', e3FileU='', e3FileV='', e3t='', e3tFile='',
                        e3Rule='', e3Static='', ssh='', sshFile='', e3Areas=''):
    """what --cell-thickness hands to Field.setCellThickness, as a tuple of its arguments, or None without the option: the
    (path, name) pairs of --e3u / --e3v, or with --e3t the one FaceThickness that derives both on the GPU from the thickness
    at T points (--e3t-file, --e3-rule, --e3-static FILE[:E3T0,E3U0,E3V0]), or with --ssh the one SshThickness that derives
    both from the sea surface height and the static thicknesses of a mesh file (--ssh-file, --e3-static MESH[:E3U0,E3V0],
    --e3-areas E1E2T,E1E2U,E1E2V); refused combinations raise RuntimeError"""
    sshArgs = checkSshArgs(cellThickness, ssh, sshFile, e3Areas, e3Static, e3t, e3tFile, e3u, e3v, e3FileU, e3FileV, e3Rule)
    if sshArgs:
        path, names, anames = sshArgs
        areas = tuple((path, n) for n in anames) if anames else None
        from .thickness import SshThickness
        return (SshThickness((sshFile or tFile, ssh), e3u0=(path, names[0]), e3v0=(path, names[1]), areas=areas),)
    if not e3t:
        if e3tFile or e3Rule or e3Static:
            raise RuntimeError('ERROR: --e3t-file / --e3-rule / --e3-static need --e3t NAME (and --cell-thickness)')
        return ((e3FileU or uFile, e3u or 'e3u'), (e3FileV or vFile, e3v or 'e3v')) if cellThickness else None
    if not cellThickness:
        raise RuntimeError('ERROR: --e3t needs --cell-thickness')
    if e3u or e3v or e3FileU or e3FileV:
        raise RuntimeError('ERROR: --e3t cannot be combined with --e3u / --e3v / --e3-file-u / --e3-file-v: the thicknesses at '
                           'the U and V points are either read or derived from --e3t')
    rule = e3Rule or 'min'
    if rule not in ('min', 'mean', 'anomaly'):
        raise RuntimeError(f'ERROR: --e3-rule must be min, mean or anomaly, got {e3Rule!r}')
    if (rule == 'anomaly') != bool(e3Static):
        raise RuntimeError('ERROR: --e3-rule anomaly and --e3-static FILE[:E3T0,E3U0,E3V0] go together')
    statics = {}
    if e3Static:
        path, sep, tail = e3Static.rpartition(':')
        names = tail.split(',') if sep and tail.count(',') == 2 and all(tail.split(',')) else None
        if names is None:
            if sep and ',' in tail:
                raise RuntimeError(f'ERROR: --e3-static must be FILE or FILE:E3T0,E3U0,E3V0 (three names), got {e3Static!r}')
            path, names = e3Static, ['e3t_0', 'e3u_0', 'e3v_0']
        statics = dict(e3t0=(path, names[0]), e3u0=(path, names[1]), e3v0=(path, names[2]))
    from .thickness import FaceThickness
    return (FaceThickness((e3tFile or tFile, e3t), rule, **statics),)


def _emit(text, output):
    if output:
        with open(output, 'w') as f:
            f.write(text)
    else:
        print(text, end='')


def checkTracerArgs(tracer='', tracerFile='', tracerRef=0.0, tracerScale=1.0, zrange=''):
    """the tracer options of the command line: refused combinations raise RuntimeError"""
    if not tracer:
        if tracerFile:
            raise RuntimeError('ERROR: --tracer-file needs --tracer NAME (the variable to read from it)')
        if float(tracerRef) != 0.0 or float(tracerScale) != 1.0:
            raise RuntimeError('ERROR: --tracer-ref / --tracer-scale need --tracer NAME')
        return
    if zrange:
        raise RuntimeError('ERROR: --tracer and --zrange cannot be combined: depth-resolved tracer transports are not '
                           'available')
    for name, x in (('--tracer-ref', tracerRef), ('--tracer-scale', tracerScale)):
        if not numpy.isfinite(float(x)):
            raise RuntimeError(f'ERROR: {name} must be a finite number, got {x!r}')


def parseZRange(zrange):
    """'ZTOP,ZBOT' -> (ztop, zbot) floats with ztop <= zbot."""
    try:
        ztop, zbot = (float(x) for x in zrange.split(','))
    except ValueError:
        raise RuntimeError(f'ERROR: --zrange must be ZTOP,ZBOT (two numbers), got {zrange!r}')
    if not ztop <= zbot:
        raise RuntimeError(f'ERROR: --zrange needs ZTOP <= ZBOT, got {zrange!r}')
    return ztop, zbot


def main(*, tFile, uFile, vFile, lonLatPoints='', iFiles='', sverdrup=False, output='', show=False, zrange='',
         tracer='', tracerFile='', tracerRef=0.0, tracerScale=1.0, classes='', levels=False, carry='', carryFile='',
         carryRef=0.0, carryScale=1.0, cellThickness=False, e3u='', e3v='', e3FileU='', e3FileV='', decompose=False,
         eddy=False, tracer2='', tracer2File='', classes2='', gross=False, thicknessWeighted=False, grossClasses='', sigma='',
         classArea='', crossings='', remap='', depthBins='', depthTop=0.0, timeWeights='', timeSelect='', depthSurfaces='',
         surfaceFile='', isoDepth='', isoOf='', isoSense='', isoRelative='', isoE3t='', mixedLayer='', grossRemap='',
         e3t='', e3tFile='', e3Rule='', e3Static='', ssh='', sshFile='', e3Areas=''):
    sig = None
    checkSshArgs(cellThickness, ssh, sshFile, e3Areas, e3Static, e3t, e3tFile, e3u, e3v, e3FileU, e3FileV, e3Rule)
    checkGrossRemapArgs(grossRemap, grossClasses, classes)
    checkTimeMeanArgs(timeWeights, timeSelect, eddy)
    iso = checkIsoDepthArgs(isoDepth, isoOf, isoSense, isoRelative, isoE3t, mixedLayer, sigma, depthSurfaces, depthTop,
                            **{'--depth-bins': depthBins, '--classes': classes, '--classes2': classes2,
                               '--gross-classes': grossClasses, '--class-area': classArea, '--crossings': crossings,
                               '--gross': gross, '--levels': levels, '--decompose': decompose, '--eddy': eddy, '--show': show,
                               '--carry': carry, '--tracer2': tracer2, '--zrange': zrange,
                               '--thickness-weighted': thicknessWeighted, '--remap': remap})
    # --surface-file and --sigma belong to --iso-depth / --mixed-layer when one of them is given
    checkDepthSurfacesArgs(depthSurfaces, '' if iso else surfaceFile, depthTop,
                           **{'--depth-bins': depthBins, '--classes': classes, '--classes2': classes2,
                              '--gross-classes': grossClasses, '--class-area': classArea, '--crossings': crossings, '--gross': gross,
                              '--levels': levels, '--decompose': decompose, '--eddy': eddy, '--show': show, '--carry': carry,
                              '--tracer2': tracer2, '--sigma': sigma, '--zrange': zrange,
                              '--thickness-weighted': thicknessWeighted, '--remap': remap})
    if depthSurfaces or iso:
        checkCellThicknessArgs(cellThickness, e3u, e3v, e3FileU, e3FileV, '', '', False, '')
        checkTracerArgs(tracer, tracerFile, tracerRef, tracerScale, '')
        lonLatZPoints, names = readTargets(lonLatPoints, iFiles)
        unit = 'Sv' if sverdrup else 'A m^2/s'
        ct = cellThicknessSource(cellThickness, tFile, uFile, vFile, e3u, e3v, e3FileU, e3FileV, e3t, e3tFile, e3Rule, e3Static,
                             ssh, sshFile, e3Areas)
        if iso:
            surfaces = iso['labels']
            totals, fld = isoSurfaceSeries(tFile, uFile, vFile, lonLatZPoints, iso, surfaceFile, float(depthTop), tracer,
                                           tracerFile, float(tracerRef), sverdrup, ct)
        else:
            surfaces = parseSurfaces(depthSurfaces)
            totals, fld = surfaceSeries(tFile, uFile, vFile, lonLatZPoints, surfaces, surfaceFile, float(depthTop), tracer,
                                        tracerFile, float(tracerRef), sverdrup, ct)
        if tracer:
            totals = totals * float(tracerScale)
            title = (f'# transport of {tracer} by layer between surfaces [{tracer} x {unit}' +
                     (f' x {float(tracerScale):g}' if float(tracerScale) != 1.0 else '') + ']')
        else:
            title = f'# water flow by layer between surfaces [{unit}]'
        title += ', depths from the cell thicknesses\n' if cellThickness else '\n'
        timeVals = [fld.timeObj.getTimeAsDate(t) for t in range(fld.nt)]
        bounds = list(zip(['top'] + surfaces, surfaces + ['bottom'])) + [('nan', 'nan')]
        lines = ['time,upper,lower,' + ','.join(names)]
        lines += [f'{timeVals[t]},{lo},{hi},' + ','.join(f'{x:.15g}' for x in totals[t, k])
                  for t in range(fld.nt) for k, (lo, hi) in enumerate(bounds)]
        _emit(title + '\n'.join(lines) + '\n', output)
        return totals
    checkDepthBinsArgs(depthBins, depthTop, **{'--classes': classes, '--classes2': classes2, '--gross-classes': grossClasses,
                                               '--class-area': classArea, '--crossings': crossings, '--gross': gross,
                                               '--levels': levels, '--decompose': decompose, '--eddy': eddy, '--show': show,
                                               '--carry': carry, '--tracer2': tracer2, '--sigma': sigma, '--zrange': zrange,
                                               '--thickness-weighted': thicknessWeighted, '--remap': remap})
    if depthBins:
        checkCellThicknessArgs(cellThickness, e3u, e3v, e3FileU, e3FileV, '', '', False, '')
        checkTracerArgs(tracer, tracerFile, tracerRef, tracerScale, '')
        lonLatZPoints, names = readTargets(lonLatPoints, iFiles)
        unit = 'Sv' if sverdrup else 'A m^2/s'
        ct = cellThicknessSource(cellThickness, tFile, uFile, vFile, e3u, e3v, e3FileU, e3FileV, e3t, e3tFile, e3Rule, e3Static,
                             ssh, sshFile, e3Areas)
        edges = parseClasses(depthBins)
        totals, fld = depthSeries(tFile, uFile, vFile, lonLatZPoints, edges, float(depthTop), tracer, tracerFile,
                                  float(tracerRef), sverdrup, ct)
        if tracer:
            totals = totals * float(tracerScale)
            title = (f'# transport of {tracer} by depth bin [{tracer} x {unit}' +
                     (f' x {float(tracerScale):g}' if float(tracerScale) != 1.0 else '') + ']')
        else:
            title = f'# water flow by depth bin [{unit}]'
        title += ', depths from the cell thicknesses\n' if cellThickness else '\n'
        timeVals = [fld.timeObj.getTimeAsDate(t) for t in range(fld.nt)]
        bounds = [(-numpy.inf, edges[0])] + list(zip(edges[:-1], edges[1:])) + [(edges[-1], numpy.inf), (numpy.nan, numpy.nan)]
        lines = ['time,ztop,zbot,' + ','.join(names)]
        lines += [f'{timeVals[t]},{lo:.15g},{hi:.15g},' + ','.join(f'{x:.15g}' for x in totals[t, k])
                  for t in range(fld.nt) for k, (lo, hi) in enumerate(bounds)]
        _emit(title + '\n'.join(lines) + '\n', output)
        return totals
    if crossings:
        checkCrossingsArgs(crossings, **{'--classes': classes, '--classes2': classes2, '--gross-classes': grossClasses,
                                         '--class-area': classArea, '--gross': gross, '--levels': levels, '--decompose': decompose,
                                         '--eddy': eddy, '--show': show, '--carry': carry, '--tracer2': tracer2,
                                         '--thickness-weighted': thicknessWeighted,
                                         '--tracer together with --sigma': bool(tracer and sigma),
                                         '--tracer-scale': float(tracerScale) != 1.0, '--remap': remap})
        checkCellThicknessArgs(cellThickness, e3u, e3v, e3FileU, e3FileV, '', '', False, '')
        lonLatZPoints, names = readTargets(lonLatPoints, iFiles)
        ct = cellThicknessSource(cellThickness, tFile, uFile, vFile, e3u, e3v, e3FileU, e3FileV, e3t, e3tFile, e3Rule, e3Static,
                             ssh, sshFile, e3Areas)
        planes, _, _ = crossingsSeries(tFile, uFile, vFile, lonLatZPoints, crossings, tracer, tracerFile, float(tracerRef),
                                       parseZRange(zrange) if zrange else None, sverdrup, ct, parseSigma(sigma) if sigma else None)
        print(f'crossings: planes of shape {planes.shape} written to {crossings}')
        return planes
    if sigma:
        # the class field computed from two variables: in the tables it goes by the name sigmaName gives it
        if tracer:
            raise RuntimeError('ERROR: --sigma and --tracer cannot be combined: --sigma THETA,SALT[,PREF] is the class field in '
                               'place of --tracer NAME')
        if not (classes or grossClasses or classes2 or classArea):
            raise RuntimeError('ERROR: --sigma needs --classes, --gross-classes or --classes2 (or --class-area): it is the class '
                               'field of the class transports (with --carry NAME too)')
        sig = parseSigma(sigma)
        tracer = sigmaName(sig[2])
    checkGrossClassArgs(grossClasses, tracer, tracerRef, tracerScale, classes, classes2, gross, levels, zrange, decompose, eddy,
                        show)
    checkClassAreaArgs(classArea, tracer, tracerRef, tracerScale, carryScale, classes, classes2, gross, grossClasses, levels,
                       zrange, decompose, eddy, show)
    checkRemapArgs(remap, classes, tracer, classes2, levels, decompose, eddy)
    checkThicknessWeightedArgs(thicknessWeighted, eddy, cellThickness)
    checkGrossArgs(gross, classes, levels, decompose, eddy, show)
    checkJointClassArgs(classes2, tracer2, tracer2File, tracer, classes, carry, levels, zrange, show, eddy, decompose)
    checkEddyArgs(eddy, tracer, classes, levels, zrange, show, decompose)
    checkDecomposeArgs(decompose, tracer, classes, levels, zrange, show)
    # --gross-classes and --class-area take --carry and --cell-thickness together: their forms have per-cell thicknesses
    checkCellThicknessArgs(cellThickness, e3u, e3v, e3FileU, e3FileV, classes, '' if grossClasses or classArea else carry, levels,
                           tracer)
    checkClassArgs(classes, tracer, tracerRef, tracerScale, zrange, show)
    checkTracerArgs(tracer, tracerFile, tracerRef, tracerScale, '' if gross else zrange)   # --gross sums its parts over a band
    checkLevelsArgs(levels, zrange, classes, show)
    checkCarryArgs(carry, carryFile, carryRef, carryScale, classes or grossClasses or classArea, tracer, levels)
    lonLatZPoints, names = readTargets(lonLatPoints, iFiles)
    print(f'target points:\n {lonLatZPoints}')
    unit = 'Sv' if sverdrup else 'A m^2/s'
    ct = cellThicknessSource(cellThickness, tFile, uFile, vFile, e3u, e3v, e3FileU, e3FileV, e3t, e3tFile, e3Rule, e3Static,
                             ssh, sshFile, e3Areas)
    if classArea:
        edges = parseClasses(classArea)
        totals, fld = classAreaSeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, tracerFile, carry, carryFile,
                                      float(carryRef), ct, sig)
        timeVals = [fld.timeObj.getTimeAsDate(t) for t in range(fld.nt)]
        bounds = [(-numpy.inf, edges[0])] + list(zip(edges[:-1], edges[1:])) + [(edges[-1], numpy.inf), (numpy.nan, numpy.nan)]
        lines = ['time,transect,lower,upper,' + ','.join(CLASS_AREA_COLUMNS)]
        lines += [f'{timeVals[t]},{name},{lo:.15g},{hi:.15g},' + ','.join(f'{x:.15g}' for x in totals[t, :, k, p])
                  for t in range(fld.nt) for p, name in enumerate(names) for k, (lo, hi) in enumerate(bounds)]
        _emit(f'# section area by {tracer} class [A m], mean {carry or tracer} of the class and depth of its upper edge\n' +
              '\n'.join(lines) + '\n', output)
        return totals
    if grossClasses:
        edges = parseClasses(grossClasses)
        series = grossRemapSeries if grossRemap else grossClassSeries
        totals, fld = series(tFile, uFile, vFile, lonLatZPoints, tracer, edges, tracerFile, carry, carryFile, float(carryRef),
                             sverdrup, ct, sig)
        title = f'# gross water flow by {tracer} class [{unit}]'
        if carry:
            totals = totals * float(carryScale)
            title = (f'# gross transport of {carry} by {tracer} class [{carry} x {unit}' +
                     (f' x {float(carryScale):g}' if float(carryScale) != 1.0 else '') + ']')
        if grossRemap:
            title += ', conservative remapping'
        timeVals = [fld.timeObj.getTimeAsDate(t) for t in range(fld.nt)]
        bounds = [(-numpy.inf, edges[0])] + list(zip(edges[:-1], edges[1:])) + [(edges[-1], numpy.inf), (numpy.nan, numpy.nan)]
        lines = ['time,transect,lower,upper,' + ','.join(GROSS_COLUMNS)]
        lines += [f'{timeVals[t]},{name},{lo:.15g},{hi:.15g},' +
                  ','.join(f'{x:.15g}' for x in (totals[t, 0, k, p], totals[t, 1, k, p], totals[t, 0, k, p] + totals[t, 1, k, p]))
                  for t in range(fld.nt) for p, name in enumerate(names) for k, (lo, hi) in enumerate(bounds)]
        _emit(title + '\n' + '\n'.join(lines) + '\n', output)
        return totals
    if gross:
        totals, fld = grossSeries(tFile, uFile, vFile, lonLatZPoints, tracer, tracerFile, float(tracerRef), float(tracerScale),
                                  parseZRange(zrange) if zrange else None, sverdrup, ct)
        timeVals = [fld.timeObj.getTimeAsDate(t) for t in range(fld.nt)]
        cols = GROSS_COLUMNS + (GROSS_TRACER_COLUMNS if tracer else ())
        title = f'# gross water flow [{unit}]'
        if tracer:
            title += (f', what it carries of {tracer} [{tracer} x {unit}' +
                      (f' x {float(tracerScale):g}' if float(tracerScale) != 1.0 else '') + f'] and its mean {tracer}')
        if zrange:
            title += f' between the depths {zrange}'
        lines = ['time,transect,' + ','.join(cols)]
        lines += [f'{timeVals[t]},{name},' + ','.join(f'{x:.15g}' for x in totals[t, p])
                  for t in range(fld.nt) for p, name in enumerate(names)]
        _emit(title + '\n' + '\n'.join(lines) + '\n', output)
        return totals
    if eddy:
        totals, fld = eddySeries(tFile, uFile, vFile, lonLatZPoints, tracer, tracerFile, float(tracerRef), sverdrup, ct,
                                 thicknessWeighted, parseTimeWeights(timeWeights) if timeWeights else None,
                                 parseTimeSelect(timeSelect) if timeSelect else None)
        nsel = len(getattr(fld, '_eddy_steps', None) or range(fld.nt))
        totals = totals * float(tracerScale)
        unit = f'{tracer} x {unit}' + (f' x {float(tracerScale):g}' if float(tracerScale) != 1.0 else '')
        lines = ['part,' + ','.join(names)]
        lines += [f'{part},' + ','.join(f'{x:.15g}' for x in totals[k]) for k, part in enumerate(EDDY_PARTS)]
        _emit(f'# mean transport of {tracer} over {nsel} time steps' + (', weighted' if timeWeights else '') +
              f', its mean-flow and eddy parts [{unit}]\n' +
              '\n'.join(lines) + '\n', output)
        return totals
    if decompose:
        totals, fld = decomposeSeries(tFile, uFile, vFile, lonLatZPoints, tracer, tracerFile, float(tracerRef), sverdrup, ct)
        totals = totals * float(tracerScale)
        unit = f'{tracer} x {unit}' + (f' x {float(tracerScale):g}' if float(tracerScale) != 1.0 else '')
        timeVals = [fld.timeObj.getTimeAsDate(t) for t in range(fld.nt)]
        lines = ['time,part,' + ','.join(names)]
        lines += [f'{timeVals[t]},{part},' + ','.join(f'{x:.15g}' for x in totals[t, k])
                  for t in range(fld.nt) for k, part in enumerate(PARTS)]
        _emit(f'# transport of {tracer} and its parts [{unit}]\n' + '\n'.join(lines) + '\n', output)
        return totals
    if levels:
        totals, fld = levelSeries(tFile, uFile, vFile, lonLatZPoints, tracer, tracerFile, float(tracerRef), sverdrup, ct)
        what = 'water flow'
        if tracer:
            totals = totals * float(tracerScale)
            what = f'transport of {tracer}'
            unit = f'{tracer} x {unit}' + (f' x {float(tracerScale):g}' if float(tracerScale) != 1.0 else '')
        timeVals = [fld.timeObj.getTimeAsDate(t) for t in range(fld.nt)]
        lines = ['time,ztop,zbot,' + ','.join(names)]
        lines += [f'{timeVals[t]},{fld.bounds_depth[z, 0]:.15g},{fld.bounds_depth[z, 1]:.15g},' +
                  ','.join(f'{x:.15g}' for x in totals[t, z]) for t in range(fld.nt) for z in range(fld.nz)]
        _emit(f'# {what} per level [{unit}]\n' + '\n'.join(lines) + '\n', output)
        return totals
    if classes2:
        edges, edges2 = parseClasses(classes), parseClasses(classes2)
        totals, fld = jointClassSeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, tracer2, edges2, tracerFile,
                                       tracer2File, sverdrup, sig)
        timeVals = [fld.timeObj.getTimeAsDate(t) for t in range(fld.nt)]

        def bounds_of(e):
            return [(-numpy.inf, e[0])] + list(zip(e[:-1], e[1:])) + [(e[-1], numpy.inf), (numpy.nan, numpy.nan)]

        lines = ['time,lower,upper,lower2,upper2,' + ','.join(names)]
        lines += [f'{timeVals[t]},{lo:.15g},{hi:.15g},{lo2:.15g},{hi2:.15g},' + ','.join(f'{x:.15g}' for x in totals[t, ka, kb])
                  for t in range(fld.nt) for ka, (lo, hi) in enumerate(bounds_of(edges))
                  for kb, (lo2, hi2) in enumerate(bounds_of(edges2))]
        _emit(f'# water flow by {tracer} class and {tracer2} class [{unit}]\n' + '\n'.join(lines) + '\n', output)
        return totals
    if classes:
        edges = parseClasses(classes)
        if remap:
            totals, fld = remapSeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, carry, tracerFile, carryFile,
                                      float(carryRef), sverdrup, sig)
        elif carry:
            totals, fld = carrySeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, carry, tracerFile, carryFile,
                                      float(carryRef), sverdrup, sig)
        else:
            totals, fld = classSeries(tFile, uFile, vFile, lonLatZPoints, tracer, edges, tracerFile, sverdrup, sig)
        if carry:
            totals = totals * float(carryScale)
            title = (f'# transport of {carry} by {tracer} class [{carry} x {unit}' +
                     (f' x {float(carryScale):g}' if float(carryScale) != 1.0 else '') + ']')
        else:
            title = f'# water flow by {tracer} class [{unit}]'
        title += ', conservative remapping\n' if remap else '\n'
        timeVals = [fld.timeObj.getTimeAsDate(t) for t in range(fld.nt)]
        bounds = [(-numpy.inf, edges[0])] + list(zip(edges[:-1], edges[1:])) + [(edges[-1], numpy.inf), (numpy.nan, numpy.nan)]
        lines = ['time,lower,upper,' + ','.join(names)]
        lines += [f'{timeVals[t]},{lo:.15g},{hi:.15g},' + ','.join(f'{x:.15g}' for x in totals[t, k])
                  for t in range(fld.nt) for k, (lo, hi) in enumerate(bounds)]
        _emit(title + '\n'.join(lines) + '\n', output)
        return totals
    if tracer:
        totals, fld = tracerSeries(tFile, uFile, vFile, lonLatZPoints, tracer, tracerFile, float(tracerRef), sverdrup, ct)
        totals = totals * float(tracerScale)
    elif zrange:
        totals, fld = bandSeries(tFile, uFile, vFile, lonLatZPoints, *parseZRange(zrange), sverdrup=sverdrup, cellThickness=ct)
    else:
        totals, fld = fluxSeries(tFile, uFile, vFile, lonLatZPoints, sverdrup, ct)
    timeVals = [fld.timeObj.getTimeAsDate(t) for t in range(fld.nt)]
    title, what = 'Water flow', 'water flow'
    if tracer:
        title = what = f'Transport of {tracer}'
        unit = f'{tracer} x {unit}' + (f' x {float(tracerScale):g}' if float(tracerScale) != 1.0 else '')
    header = 'time,' + ','.join(names)
    lines = [header] + [f'{timeVals[t]},' + ','.join(f'{x:.15g}' for x in totals[t]) for t in range(fld.nt)]
    if output:
        with open(output, 'w') as f:
            f.write(f'# {what} [{unit}]\n' + '\n'.join(lines) + '\n')
    else:
        print(f'# {what} [{unit}]')
        print('\n'.join(lines))
    if show:
        try:
            import matplotlib.pyplot as plt
        except ImportError:
            print('# matplotlib is not installed: no plot')
            return totals
        lineTypes = ['b-', 'm--', 'c-.', 'r:', 'g-', 'k--']  # fluxplot.py:62
        for i, name in enumerate(names):
            plt.plot(timeVals, totals[:, i], lineTypes[i % len(lineTypes)])
        if len(names) > 1:
            plt.legend(names)
        plt.title(title)
        plt.ylabel(unit)
        plt.show()
    return totals


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description='Flux time series across transects (GPU batch driver)')
    ap.add_argument('-t', '--tFile', required=True)
    ap.add_argument('-u', '--uFile', required=True)
    ap.add_argument('-v', '--vFile', required=True)
    ap.add_argument('-l', '--lonLatPoints', default='')
    ap.add_argument('-i', '--iFiles', default='')
    ap.add_argument('-s', '--sverdrup', action='store_true')
    ap.add_argument('-o', '--output', default='')
    ap.add_argument('--show', action='store_true')
    ap.add_argument('--zrange', default='', metavar='ZTOP,ZBOT',
                    help='flux inside this depth band only (units of deptht_bounds), one depth-resolved step per time step')
    ap.add_argument('--tracer', default='', metavar='NAME',
                    help='tracer transport (e.g. heat: thetao) instead of the water flow: NAME is read from the T file')
    ap.add_argument('--tracer-file', dest='tracerFile', default='', metavar='FILE', help='read --tracer from FILE instead')
    ap.add_argument('--tracer-ref', dest='tracerRef', type=float, default=0.0, metavar='X',
                    help='reference value subtracted from the tracer (theta_ref of a heat transport across an open section)')
    ap.add_argument('--tracer-scale', dest='tracerScale', type=float, default=1.0, metavar='S',
                    help='multiply the tracer transport by S (with -s: 1e6 * rho0 * c_p * 1e-15 = 4.1e-3 turns Sv degC into PW)')
    ap.add_argument('--sigma', default='', metavar='THETA,SALT[,PREF]',
                    help='in place of --tracer NAME as the class field of --classes, --gross-classes, --carry and --classes2: '
                         'the potential density sigma_PREF (EOS-80; PREF in dbar, default 0) of potential temperature THETA and '
                         'practical salinity SALT, computed on the GPU one time step at a time; the two are read from the T '
                         'file, or from --tracer-file')
    ap.add_argument('--classes', default='', metavar='E0,E1,...,EN',
                    help='water flow binned by the class of --tracer NAME (e.g. sigma0): one CSV line per time step and '
                         'class [-inf,E0), [E0,E1), ..., [EN,inf), and a last one (nan,nan) for faces without a value')
    ap.add_argument('--remap', default='', metavar='linear',
                    help='with --classes (and --carry): conservative remapping -- a level\'s transport is spread over the '
                         'classes between the class field\'s values at the layer\'s upper and lower interface (piecewise-linear '
                         'in z) instead of going whole to the class of its face: a smooth MOC(sigma) with many class edges')
    ap.add_argument('--depth-bins', dest='depthBins', default='', metavar='E0,E1,...,EN',
                    help='water flow in true-depth bins: one CSV line per time step and bin [-inf,E0), [E0,E1), ..., [EN,inf), '
                         'and a last one (nan,nan) for layers without a finite depth.  A level\'s transport is spread over the '
                         'bins that its layer covers at each face; with --cell-thickness the layer depths are the running sum '
                         'of e3u / e3v at the face (partial steps, z*, s-coordinates).  With --tracer NAME the transport of NAME '
                         '(--tracer-ref, --tracer-scale apply); -s applies')
    ap.add_argument('--depth-top', dest='depthTop', type=float, default=0.0, metavar='X',
                    help='with --depth-bins or --depth-surfaces: the depth of the upper interface of the first level (default 0)')
    ap.add_argument('--depth-surfaces', dest='depthSurfaces', default='', metavar='NAME[,NAME...]',
                    help='water flow in the layers bounded by 1 to 8 two-dimensional variables at T-points (mixed-layer depth, '
                         'the depth of an isotherm, column depth minus 200): one CSV line per time step and layer -- above the '
                         'first surface, between consecutive surfaces, below the last, and a last one (nan,nan) for faces where '
                         'a surface has no value.  Depths are positive downward from --depth-top; a surface that rises above '
                         'the one before it is taken at that one.  With --tracer NAME the transport of that variable; with '
                         '--cell-thickness the layer depths are the running sum of e3u / e3v')
    ap.add_argument('--surface-file', dest='surfaceFile', default='', metavar='FILE',
                    help='with --depth-surfaces: the file that holds the surfaces (default: the T file)')
    ap.add_argument('--iso-depth', dest='isoDepth', default='', metavar='V1[,...,Vm]',
                    help='the table of --depth-surfaces with surfaces computed on the GPU, one time step at a time: the depths at '
                         'which the variable of --iso-of NAME, or the potential density of --sigma THETA,SALT[,PREF], first '
                         'reaches each of the 1 to 8 values going down the column (linear between level centres; the sea bed '
                         'where it never does, --depth-top where level 0 already has).  The variables are read from the T file, '
                         'or from --surface-file.  --depth-top, --tracer, --cell-thickness and -s apply as with '
                         '--depth-surfaces; refused together with it')
    ap.add_argument('--iso-of', dest='isoOf', default='', metavar='NAME', help='with --iso-depth: the variable (e.g. thetao)')
    ap.add_argument('--iso-sense', dest='isoSense', default='', metavar='rising|falling',
                    help='with --iso-depth: whether the variable rises downward (density; the default with --sigma) or falls '
                         '(temperature; the default with --iso-of)')
    ap.add_argument('--iso-relative', dest='isoRelative', default='', metavar='ZREF',
                    help="with --iso-depth: the values are offsets from the variable's own value at depth ZREF (a threshold "
                         "criterion: --iso-of thetao --iso-depth -0.2 --iso-relative 10)")
    ap.add_argument('--iso-e3t', dest='isoE3t', default='', metavar='NAME',
                    help='with --iso-depth or --mixed-layer: the cell thicknesses at T-points, a variable of the same file '
                         '(partial steps, z*); default: the level thicknesses of deptht_bounds')
    ap.add_argument('--mixed-layer', dest='mixedLayer', default='', metavar='THETA,SALT[,DELTA[,ZREF]]',
                    help='the table of --depth-surfaces with one surface, the mixed-layer depth: where sigma0 of THETA and SALT '
                         'first exceeds its value at ZREF (default 10) by DELTA (default 0.03 kg m-3)')
    ap.add_argument('--tracer2', default='', metavar='NAME',
                    help='with --classes2: the second class field (e.g. so beside --tracer thetao); NAME is read from the T file')
    ap.add_argument('--tracer2-file', dest='tracer2File', default='', metavar='FILE', help='read --tracer2 from FILE instead')
    ap.add_argument('--classes2', default='', metavar='F0,F1,...,FM',
                    help='with --tracer NAME --classes E0,...,EN and --tracer2 NAME: the water flow in joint classes of the two '
                         'tracers (a T-S census): one CSV line per time step and pair of classes')
    ap.add_argument('--carry', default='', metavar='NAME',
                    help='with --classes: the transport of tracer NAME (e.g. heat: thetao) by class of --tracer, in place of '
                         'the water flow; NAME is read from the T file')
    ap.add_argument('--carry-file', dest='carryFile', default='', metavar='FILE', help='read --carry from FILE instead')
    ap.add_argument('--carry-ref', dest='carryRef', type=float, default=0.0, metavar='X',
                    help='reference value subtracted from the carried tracer')
    ap.add_argument('--carry-scale', dest='carryScale', type=float, default=1.0, metavar='S',
                    help='multiply the carried transport by S')
    ap.add_argument('--levels', action='store_true',
                    help='one CSV line per time step and level (time,ztop,zbot,...): the water flow of each level, or with '
                         '--tracer NAME the transport of NAME of each level (--tracer-ref, --tracer-scale apply)')
    ap.add_argument('--decompose', action='store_true',
                    help='with --tracer NAME: one CSV line per time step and part (time,part,...): the transport of NAME and its '
                         'throughflow, overturning and gyre parts (--tracer-ref, --tracer-scale, -s and --cell-thickness apply)')
    ap.add_argument('--gross', action='store_true',
                    help='one CSV line per time step and transect (time,transect,inflow,outflow,net): the water that crosses in '
                         'the positive direction, the water that comes back, and their sum; with --tracer NAME also what the two '
                         'carry of NAME and the transport-weighted mean NAME of each (--zrange, --cell-thickness, --tracer-ref, '
                         '--tracer-scale and -s apply)')
    ap.add_argument('--gross-classes', dest='grossClasses', default='', metavar='E0,E1,...,EN',
                    help='with --tracer NAME (the class field): one CSV line per time step, transect and class '
                         '(time,transect,lower,upper,inflow,outflow,net): the water of that class that crosses in the positive '
                         'direction, the water that comes back, and their sum; with --carry NAME what the two carry of NAME '
                         '(--carry-ref, --carry-scale, --cell-thickness and -s apply)')
    ap.add_argument('--gross-remap', dest='grossRemap', default='', metavar='linear',
                    help='with --gross-classes (and --carry, --cell-thickness, --sigma): conservative remapping -- a level\'s '
                         'inflow and outflow are spread over the classes between the class field\'s values at the layer\'s two '
                         'interfaces instead of going whole to one class: smooth inflow, outflow and net (MOC) with many classes, '
                         'under per-cell thicknesses too')
    ap.add_argument('--class-area', dest='classArea', default='', metavar='E0,E1,...,EN',
                    help='with --tracer NAME or --sigma (the class field): one CSV line per time step, transect and class '
                         '(time,transect,lower,upper,area,mean,depth): the section area that the class occupies, the '
                         'area-weighted mean of the class field in it -- with --carry NAME of NAME (--carry-ref applies) -- and '
                         'the pseudo-depth of the upper edge of the class, the depth axis of an overturning streamfunction in '
                         'class space (--cell-thickness applies; -s does not: an area has no Sverdrup scale)')
    ap.add_argument('--crossings', default='', metavar='FILE.npz',
                    help='write the per-crossing planes of every time step to FILE.npz: what flows through the piece of the line '
                         'inside each grid cell at each level (q) and its section area (g); with --tracer NAME or --sigma the '
                         'carried form (q, c, a, b).  Also the position of every crossing along the line and the cumulative '
                         'transport (--zrange: of that band).  With --cell-thickness, -s, --tracer-ref.  Refused above 2 GiB')
    ap.add_argument('--eddy', action='store_true',
                    help='with --tracer NAME: one CSV line per part (part,...): the mean over all time steps of the transport of '
                         'NAME, the transport of the time-mean NAME by the time-mean flow, and the eddy part, their difference '
                         '(--tracer-ref, --tracer-scale, -s apply)')
    ap.add_argument('--time-weights', dest='timeWeights', default='', metavar='bounds|W0,W1,...',
                    help="with --eddy: the weights of the steps of the time mean, 'bounds' for the step lengths of the time "
                         "variable's bounds (months of 28 to 31 days) or one positive number per visited step")
    ap.add_argument('--time-select', dest='timeSelect', default='', metavar='I0,I1,...|months:M1,M2,...',
                    help='with --eddy: the steps of the time mean, as ascending step indices or as the months (1-12) to keep '
                         '(months:12,1,2 is DJF of every year)')
    ap.add_argument('--cell-thickness', dest='cellThickness', action='store_true',
                    help='integrate with per-cell layer thicknesses (partial steps, z*) read from the U and V files instead of '
                         'deptht_bounds; with the plain series, --zrange, --levels (without --tracer) and --tracer NAME')
    ap.add_argument('--thickness-weighted', dest='thicknessWeighted', action='store_true',
                    help='with --eddy and --cell-thickness, for thicknesses that change with time (z*, variable volume): the '
                         'mean flow is the mean thickness times the thickness-weighted mean velocity, so that it carries the '
                         'mean volume transport')
    ap.add_argument('--e3u', default='', metavar='NAME', help='with --cell-thickness: the thickness at U points (default e3u)')
    ap.add_argument('--e3v', default='', metavar='NAME', help='with --cell-thickness: the thickness at V points (default e3v)')
    ap.add_argument('--e3-file-u', dest='e3FileU', default='', metavar='FILE', help='read --e3u from FILE instead of the U file')
    ap.add_argument('--e3-file-v', dest='e3FileV', default='', metavar='FILE', help='read --e3v from FILE instead of the V file')
    ap.add_argument('--e3t', default='', metavar='NAME',
                    help='with --cell-thickness: derive the thicknesses at the U and V points on the GPU from the thickness NAME at '
                         'T points (e3t, thkcello) of the T file, instead of reading --e3u / --e3v')
    ap.add_argument('--e3t-file', dest='e3tFile', default='', metavar='FILE', help='read --e3t from FILE instead of the T file')
    ap.add_argument('--e3-rule', dest='e3Rule', default='', metavar='min|mean|anomaly',
                    help='with --e3t: the face takes the thinner of its two cells (min, the default: partial steps), their mean, '
                         'or the static face thickness plus the mean anomaly of the two cells (anomaly: z*; needs --e3-static)')
    ap.add_argument('--e3-static', dest='e3Static', default='', metavar='FILE[:E3T0,E3U0,E3V0]',
                    help='with --e3-rule anomaly: the mesh file that holds the static thicknesses at the T, U and V points '
                         '(default names e3t_0,e3u_0,e3v_0)')
    ap.add_argument('--ssh', default='', metavar='NAME',
                    help='with --cell-thickness, for z* output that holds no 3-D thickness: derive the thicknesses at the U and V '
                         'points on the GPU from the sea surface height NAME (ssh, zos) of the T file and the static thicknesses '
                         'of --e3-static MESH[:E3U0,E3V0] (default names e3u_0,e3v_0): e3u_0 * (1 + ssh_u / hu_0)')
    ap.add_argument('--ssh-file', dest='sshFile', default='', metavar='FILE', help='read --ssh from FILE instead of the T file')
    ap.add_argument('--e3-areas', dest='e3Areas', default='', metavar='E1E2T,E1E2U,E1E2V',
                    help="with --ssh: the cell areas at the T, U and V points in the mesh file of --e3-static, for NEMO's "
                         'area-weighted sea surface height at the faces (default: the plain mean of the two cells)')
    main(**vars(ap.parse_args()))
