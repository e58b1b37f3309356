"""Cost of the crossings (nf_field_compute_crossings_async) against the existing passes that yield the same planes' segment
sums, in one process.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects, nt = 2; the inputs of
tools/gross_timing.py), float64 and float32, inputs in HBM; ms per call, HIP events on the handle's stream, median with min and
max of --reps repetitions after warm-up, the calls of one comparison alternating:
  * both forms -- volume (q, g) and carried (q, c, a, b) -- with the scalar and a static per-cell thickness, with every chunk
    length (the "crossing_chunk" knob) and with the default;
  * their bars, the cost of getting the same planes from separate existing passes: 2 x nf_field_compute_profile for the
    volume form; nf_field_compute_profile + nf_field_compute_tracer_profile + nf_field_compute_area_profile for the carried
    form, with nf_field_compute_gross_profile(carry = 1) in the middle when a cell thickness is set;
  * the worst |err| / mag of the device planes against tests/crossings_reference.py for one step (float64, scalar thickness),
    the values gathered from HBM level by level, and how many values differ in their bits.

    python tools/crossings_timing.py [--reps N] [--dtype f64|f32] [--no-host] [--out FILE]
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy  # noqa: E402
import torch  # noqa: E402

from gross_timing import FILL, NX, NY, NZ, NT, REF, Handle, fmt, inputs, timed  # noqa: E402
from nemoflux_amd import _lib  # noqa: E402

CHUNKS = (2, 4, 8)


def measure(real, args, say):
    a = inputs(real)
    me = Handle(_lib.lib, a)
    n = ctypes.c_size_t()
    me.call('num_crossings', ctypes.byref(n))
    nrec = n.value
    say(f'== bench {NX} x {NY} x {NZ} {real}, nt = {NT}, {len(a["lines"])} transects, {nrec} crossings, row length {me.rowlen}; '
        f'medians of {args.reps} (min - max), ms per call')
    out = torch.zeros((4, NZ, nrec), dtype=torch.float64, device='cuda')
    rows = torch.zeros((2, NZ, me.rowlen), dtype=torch.float64, device='cuda')
    p_out, p_rows = ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(rows.data_ptr())

    def crossings(carry):
        return lambda: me.call('compute_crossings_async', 0, carry, p_out)

    def net(name, *extra):
        return lambda: me.call(name + '_async', 0, *extra, p_rows)

    for ct in (False, True):
        me.cell_thickness(a, ct)
        th = 'cell thickness  ' if ct else 'scalar thickness'
        middle = ('compute_gross_profile', 1) if ct else ('compute_tracer_profile',)
        yards = [net('compute_profile'), net(*middle), net('compute_area_profile')]
        names = ['nf_field_compute_profile', 'nf_field_' + middle[0] + ('(carry = 1)' if ct else ''), 'nf_field_compute_area_profile']
        for carry, form in ((0, 'volume'), (1, 'carried')):
            best = None
            for chunk in CHUNKS + (0,):
                assert _lib.lib.nf_tuning_set(b'crossing_chunk', chunk) == 0
                t = timed([crossings(carry)] + yards, args.reps)
                bar = 2. * t[1][0] if not carry else t[1][0] + t[2][0] + t[3][0]
                label = f'{chunk} levels per chunk' if chunk else 'DEFAULT chunk     '
                say(f'crossings  {form:<8s} {th}  {label}   {fmt(t[0])}   = {t[0][0] / bar:.2f} x its bar ({bar:.3f} ms: '
                    + (f'2 x {t[1][0]:.3f}' if not carry else ' + '.join(f'{x[0]:.3f}' for x in t[1:])) + ')'
                    + ('' if chunk else f': {"met" if t[0][0] <= bar else "MISSED"}'))
                if chunk and (best is None or t[0][0] < best[1]):
                    best = (chunk, t[0][0])
            say(f'           {form:<8s} {th}  fastest candidate: {best[0]} levels per chunk')
        for nm, x in zip(names, timed(yards, args.reps)):
            say(f'yardstick  {nm:<42s} {th}  {fmt(x)}')
    me.cell_thickness(a, False)
    assert _lib.lib.nf_tuning_set(b'crossing_chunk', 0) == 0
    if real == 'float64' and not args.no_host:
        from crossings_reference import PLANES, CrossingsReference
        arc = numpy.zeros((NY * NX, 4))
        me.call('get_arclengths', arc.ctypes.data_as(_lib.c_double_p))
        ce, w, sg = me.weights()
        tr_off = numpy.concatenate([[0], numpy.cumsum([len(x) - 1 for x in a['lines']])])
        t0 = time.time()
        ref = CrossingsReference(ce, w, sg, arc, a['th'], tr_off, NX, NY, uv_markers=(FILL,), reference=REF, wrap=True, sverdrup=True)
        cells = torch.from_numpy(ref.cells).cuda()

        def values(name, zz, c):
            return a[name][0, zz].reshape(-1)[cells].cpu().numpy()

        for carry in (0, 1):
            want, mag = ref.crossing_step(values, bool(carry))
            crossings(carry)()
            torch.cuda.synchronize()
            got = out[:want.shape[0]].cpu().numpy()
            for p, nm in enumerate(PLANES[bool(carry)]):
                ratio = float((numpy.abs(got[p] - want[p]) / numpy.maximum(mag[p], 1e-300)).max())
                differ = int((got[p].view(numpy.uint64) != want[p].view(numpy.uint64)).sum())
                say(f'reference  {"carried" if carry else "volume":<8s} plane {nm}: worst |err| / mag = {ratio:.3g} (bar 4 eps = '
                    f'{4 * numpy.finfo(float).eps:.3g}), {differ} of {got[p].size} values differ in their bits')
        say(f'host reference of one step, both forms (numpy): {time.time() - t0:.1f} s')
    me.call('del')
    del a
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--no-host', dest='no_host', action='store_true', help='skip the comparison with the host reference')
    ap.add_argument('--out', default='', help='also append the lines to this file')
    args = ap.parse_args()

    def say(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')
    for dt, real in (('f64', 'float64'), ('f32', 'float32')):
        if args.dtype and dt != args.dtype:
            continue
        measure(real, args, say)


if __name__ == '__main__':
    main()
