"""A model of everything one nf_field handle of the C ABI carries (Level 2 of include/nemoflux_amd.h), for the handle re-use
tests: random setter calls in any order, the ten compute kinds, and for every compute what the header promises -- "the same
as a fresh handle given the final state alone" or "refused with code C".  Pure numpy: nothing here touches a GPU, so the
generator itself is checked on the CPU (tests/test_reuse_model_cpu.py) with a handle that only records its calls; the GPU
test (tests/test_gpu_reuse_products.py) passes a handle that forwards them to the library.

The handle the model drives has these methods (arrays are numpy arrays; the handle uploads the ones that go to HBM and keeps
every borrowed array alive): set_stream(index 0..2), set_bounds(ny, nx, dtype, on_device), set_thickness(thick),
set_uv(u, v, on_device, fill), add_transect(points), set_tracer(a, on_device, fill), set_class_tracer(a or None, on_device,
fill), set_class_edges(edges), set_cell_thickness(e3u or None, e3v, on_device, fill) and call(name, *scalars) for the rest.

Refusals, from the header alone (codes NF_ERR_ARG = 1, NF_ERR_STATE = 2):
    no_tracer, no_edges   a tracer / class form before set_tracer / set_class_edges                          STATE
    no_weights            any form but compute_flux after add_transect or set_bounds, before build_weights   STATE
    ct_set                a form that takes no cell thickness while one is set                               STATE
    tracer_mismatch, sig_mismatch, ct_mismatch
                          dtype or nt no longer those of uo/vo after a later set_uv                          ARG
    ct_stale              a static host cell thickness uploaded for another (nz, ny, nx)                     STATE
Where several hold the header gives no precedence: any of their codes is accepted, success never.

What the library cannot refuse it is never asked to do: a borrowed array (uo/vo, tracer, class tracer, HBM or time-varying
cell thickness) whose (nz, ny, nx) no longer fits carries no shape in its call, so ready() always sets it again before a
compute that reads it.  ready() is lazy only about the steps that would remove a documented refusal."""
import numpy

from test_gpu_reuse import GRIDS, TRANSECTS      # (that module imports nothing of the GPU until a test runs)

NF_ERR_ARG, NF_ERR_STATE = 1, 2
FILL, MISSING = 1.e20, -999.              # the two markers every array may carry (when its setters name them)

KINDS = ['flux', 'all', 'read', 'profile', 'tracer_flux', 'tracer_all', 'class_transport', 'tracer_profile', 'area_profile',
         'class_tracer_transport']
BOTH_FORMS = {'profile', 'class_transport', 'tracer_profile', 'area_profile', 'class_tracer_transport'}
READS_TRACER = {'tracer_flux', 'tracer_all', 'class_transport', 'tracer_profile', 'area_profile', 'class_tracer_transport'}
CLASS_KINDS = {'class_transport', 'class_tracer_transport'}
NO_CELL_THICK = {'tracer_profile', 'class_transport', 'class_tracer_transport'}
READS_CELL_THICK = {'flux', 'all', 'read', 'profile', 'tracer_flux', 'tracer_all', 'area_profile'}
NEEDS_NO_WEIGHTS = {'flux', 'read'}
CODES = {'no_tracer': NF_ERR_STATE, 'no_edges': NF_ERR_STATE, 'no_weights': NF_ERR_STATE, 'ct_set': NF_ERR_STATE,
         'tracer_mismatch': NF_ERR_ARG, 'sig_mismatch': NF_ERR_ARG, 'ct_mismatch': NF_ERR_ARG, 'ct_stale': NF_ERR_STATE}
# the refusal classes of the issue -> the causes above
REFUSAL_CLASSES = {'missing_input': ('no_tracer', 'no_edges'), 'no_weights': ('no_weights',), 'ct_set': ('ct_set',),
                   'tracer_mismatch': ('tracer_mismatch',), 'sig_mismatch': ('sig_mismatch',), 'ct_mismatch': ('ct_mismatch',),
                   'ct_stale': ('ct_stale',)}

CT_HOMES = {'ct_static_host': (True, False), 'ct_static_hbm': (True, True), 'ct_tv_host': (False, False),
            'ct_tv_hbm': (False, True)}          # op -> (static, on_device)
SETTERS = ['bounds', 'thickness', 'uv', 'missing', 'sverdrup', 'compact', 'slab', 'transect', 'stream0', 'stream1', 'stream2',
           'tracer', 'tracer_missing', 'tracer_ref', 'tracer_wrap', 'sig', 'sig_missing', 'sig_clear', 'edges',
           'ct_static_host', 'ct_static_hbm', 'ct_tv_host', 'ct_tv_hbm', 'ct_missing', 'ct_clear']
# draw weights: the ops that ready() makes on its own account as well are drawn less often than the rest, the static host cell
# thickness more often (the one home whose upload can go stale), and about two ops in five are computes
WEIGHTS = dict({op: 1.0 for op in SETTERS}, bounds=0.5, thickness=0.5, uv=0.6, transect=0.4, tracer=0.4, ct_clear=0.5, edges=0.7,
               ct_static_host=1.6, ct_tv_hbm=1.3, compute=13.0)
KIND_WEIGHTS = dict({k: 1.0 for k in KINDS}, all=1.8, class_transport=1.3, class_tracer_transport=1.5, read=0.7, tracer_flux=1.3,
                    tracer_profile=1.3)
# the setters that change what a pass launches (the header: they invalidate a captured pass); build_weights does too.  The
# tracer, class tracer and class edge setters and add_transect do not.
VERSION_OPS = {'bounds', 'thickness', 'uv', 'missing', 'sverdrup', 'compact', 'slab', 'stream0', 'stream1', 'stream2',
               'ct_static_host', 'ct_static_hbm', 'ct_tv_host', 'ct_tv_hbm', 'ct_missing', 'ct_clear'}
# set_uv is drawn this much more often under a class tracer that fits; uo / vo go to HBM this often (a pass is captured there)
UV_UNDER_SIG, UV_HBM = 5.0, 0.7
LAZY = 0.5            # how often ready() leaves the pending refusals in place
SEEDS = list(range(16))      # the sequences of the GPU test; tests/test_reuse_model_cpu.py holds what they must cover
NOPS = 28


def land_array(rng, shape, dtype, fill, lo=None, hi=None, zeros=False):
    """(nt, nz, ny, nx) values of dtype -- normal, or uniform in [lo, hi) -- with land: columns of `fill` (when there is one),
    columns of NaN and columns of the second marker; `zeros`: some cells are exactly 0 (a thickness)."""
    a = rng.standard_normal(shape) if lo is None else rng.uniform(lo, hi, shape)
    a = a.astype(dtype)
    ny, nx = shape[2:]
    if zeros:
        a[rng.random(shape) < 0.1] = 0
    land = rng.random((ny, nx))
    if fill is not None:
        a[:, :, land < 0.10] = dtype(fill)
    a[:, :, (land >= 0.10) & (land < 0.14)] = numpy.nan
    a[:, :, (land >= 0.14) & (land < 0.18)] = dtype(MISSING)
    return a


class Model:
    """The state a sequence of setter calls leaves.  apply() draws and makes one setter call, ready() the calls that a compute
    needs, plan() says what the compute must give, fresh() repeats the final state on a new handle.  `log` keeps what was
    done: ('set', op) and ('compute', plan)."""

    def __init__(self, rng, lazy=LAZY):
        self.rng, self.lazy, self.log = rng, lazy, []
        self.grid = None            # (ny, nx, dtype, on_device)
        self.thick = None
        self.uv = None              # (u, v, on_device, fill)
        self.missing = None
        self.sverdrup = 0
        self.compact = 0
        self.slab = None
        self.transects = []
        self.weights_built = False
        self.stream = 0
        self.tracer = None          # (a, on_device, fill)
        self.tracer_missing, self.tracer_ref, self.tracer_wrap = None, 0.0, 1
        self.sig = None             # (a, on_device, fill)
        self.sig_missing = None
        self.edges = None
        self.ct = None              # (e3u, e3v, on_device, fill, static)
        self.ct_missing = None
        # a captured pass: `version` counts the calls that invalidate one, `captured` is the version at the latest capturable
        # 'all' (None: none yet), `between` the tracer / class setters and other computes since then
        self.version, self.captured, self.between = 0, None, 0
        self.all_seen = False                 # an 'all' has succeeded on this handle ...
        self.tracer_set_after_all = False     # ... and a tracer setter came after the latest one

    # ---- shapes ------------------------------------------------------------------------------------------------------------
    def shape3(self):
        return (self.thick.size,) + tuple(self.grid[:2])

    def steps(self):
        return self.uv[0].shape[0]

    def _fits(self, a, nt):
        """'ok', 'mismatch' (dtype or nt differ from uo/vo: refused with NF_ERR_ARG) or 'stale' ((nz, ny, nx) differ:
        nothing in the call says so)"""
        u = self.uv[0]
        if a.dtype != u.dtype or nt != u.shape[0]:
            return 'mismatch'
        return 'ok' if a.shape[1:] == self.shape3() else 'stale'

    def tracer_state(self):
        return 'none' if self.tracer is None else self._fits(self.tracer[0], self.tracer[0].shape[0])

    def sig_state(self):
        return 'none' if self.sig is None else self._fits(self.sig[0], self.sig[0].shape[0])

    def ct_state(self):
        """as _fits, and 'owned_stale' for a static host array (uploaded at the call) of another (nz, ny, nx), whatever its
        dtype"""
        if self.ct is None:
            return 'none'
        e3u, _, on_device, _, static = self.ct
        if static and not on_device and e3u.shape[1:] != self.shape3():
            return 'owned_stale'
        return self._fits(e3u, self.steps() if static else e3u.shape[0])

    def ct_mismatch(self):
        if self.ct is None:
            return False
        e3u, static = self.ct[0], self.ct[4]
        return e3u.dtype != self.uv[0].dtype or (not static and e3u.shape[0] != self.steps())

    def ct_home(self):
        if self.ct is None:
            return None
        return ('ct_static_' if self.ct[4] else 'ct_tv_') + ('hbm' if self.ct[2] else 'host')

    # ---- setters -----------------------------------------------------------------------------------------------------------
    def draw_op(self):
        names = SETTERS + ['compute']
        p = numpy.array([WEIGHTS[n] for n in names])
        if self.ct_home() == 'ct_static_host':       # the upload that a change of the shape leaves stale: change it more often
            p[names.index('bounds')] *= 6
            p[names.index('thickness')] *= 6
        if self.sig is not None and self.uv is not None and self.sig_state() == 'ok':
            p[names.index('uv')] *= UV_UNDER_SIG     # a later set_uv under a class tracer: its dtype / nt refusal
        if self.stream == 0:                         # graphs are captured on the other two
            p[names.index('stream1')] *= 2
            p[names.index('stream2')] *= 2
        if self.uv is not None and ('mismatch' in (self.sig_state(), self.tracer_state()) or self.ct_state() == 'owned_stale'):
            p[names.index('compute')] *= 2           # a refusal is pending: ask for it before another setter removes it
        if self.captured == self.version:            # a captured pass is alive: let it live to be replayed
            for op in VERSION_OPS:
                p[names.index(op)] *= 0.3
        return names[self.rng.choice(len(names), p=p / p.sum())]

    def _marker(self):
        return [None, MISSING][self.rng.integers(2)]

    @staticmethod
    def _nan(x):
        return float('nan') if x is None else x

    def need_uv(self, h):
        if self.grid is None:
            self.apply(h, 'bounds')
        if self.thick is None:
            self.apply(h, 'thickness')
        if self.uv is None:
            self.apply(h, 'uv')

    def apply(self, h, op):
        rng = self.rng
        if op == 'bounds':
            ny, nx = GRIDS[rng.integers(len(GRIDS))]
            self.grid = (ny, nx, [numpy.float64, numpy.float32][rng.integers(2)], bool(rng.integers(2)))
            self.weights_built = False
            h.set_bounds(*self.grid)
        elif op == 'thickness':
            self.thick = rng.uniform(1., 50., int(rng.integers(1, 8)))
            h.set_thickness(self.thick)
        elif op == 'uv':
            if self.grid is None:
                self.apply(h, 'bounds')
            if self.thick is None:
                self.apply(h, 'thickness')
            dtype = [numpy.float64, numpy.float32][rng.integers(2)]
            fill = [None, FILL][rng.integers(2)]
            shape = (int(rng.choice([1, 2, 2, 3, 3])),) + self.shape3()    # nt = 1 has no time-varying thickness
            self.uv = (land_array(rng, shape, dtype, fill), land_array(rng, shape, dtype, fill), bool(rng.random() < UV_HBM), fill)
            h.set_uv(*self.uv)
        elif op == 'missing':
            self.missing = self._marker()
            h.call('set_missing_value', self._nan(self.missing))
        elif op == 'sverdrup':
            self.sverdrup = int(rng.integers(2))
            h.call('set_sverdrup', self.sverdrup)
        elif op == 'compact':
            self.compact = int(rng.integers(2))
            h.call('set_compact', self.compact)
        elif op == 'slab':
            total = self.steps() * self.thick.size if self.uv is not None and self.thick is not None else 8
            b = int(rng.integers(0, total))
            self.slab = (b, int(rng.integers(b + 1, total + 1)))
            h.call('set_slab_range', *self.slab)
        elif op == 'transect':
            self.transects.append(TRANSECTS[rng.integers(len(TRANSECTS))])
            self.weights_built = False
            h.add_transect(self.transects[-1])
        elif op.startswith('stream'):
            self.stream = int(op[-1])
            h.set_stream(self.stream)
        elif op == 'tracer':
            self.need_uv(h)
            u = self.uv[0]
            fill = [None, FILL][rng.integers(2)]
            # values on both sides of every class edge (edges lie in [2, 8])
            a = land_array(rng, (u.shape[0],) + self.shape3(), u.dtype.type, fill, 0., 10.)
            self.tracer = (a, bool(rng.integers(2)), fill)
            h.set_tracer(*self.tracer)
            self.tracer_set_after_all = self.all_seen
        elif op == 'tracer_missing':
            self.tracer_missing = self._marker()
            h.call('set_tracer_missing_value', self._nan(self.tracer_missing))
            self.tracer_set_after_all = self.all_seen
        elif op == 'tracer_ref':
            self.tracer_ref = [0.0, 3.5, -2.0][rng.integers(3)]
            h.call('set_tracer_reference', self.tracer_ref)
            self.tracer_set_after_all = self.all_seen
        elif op == 'tracer_wrap':
            self.tracer_wrap = int(rng.integers(2))
            h.call('set_tracer_wrap', self.tracer_wrap)
            self.tracer_set_after_all = self.all_seen
        elif op == 'sig':
            self.need_uv(h)
            u = self.uv[0]
            fill = [None, FILL][rng.integers(2)]
            a = land_array(rng, (u.shape[0],) + self.shape3(), u.dtype.type, fill, 0., 10.)
            self.sig = (a, bool(rng.integers(2)), fill)
            h.set_class_tracer(*self.sig)
        elif op == 'sig_missing':
            self.sig_missing = self._marker()
            h.call('set_class_tracer_missing_value', self._nan(self.sig_missing))
        elif op == 'sig_clear':                      # NULL: the class field is the tracer again, the markers are forgotten
            self.sig, self.sig_missing = None, None
            h.set_class_tracer(None, False, None)
        elif op == 'edges':
            n = int(rng.integers(2, 7))
            self.edges = numpy.sort(rng.choice(numpy.arange(2., 8., 0.25), n, replace=False))
            h.set_class_edges(self.edges)
        elif op in CT_HOMES:
            self.need_uv(h)
            static, on_device = CT_HOMES[op]
            u = self.uv[0]
            if u.shape[0] == 1:
                static = True                        # nt_th == nt == 1 is a static thickness, whatever it was meant to be
                op = 'ct_static_' + ('hbm' if on_device else 'host')
            fill = [None, FILL][rng.integers(2)]
            shape = (1 if static else u.shape[0],) + self.shape3()
            e3u, e3v = (land_array(rng, shape, u.dtype.type, fill, 0.5, 40., zeros=True) for _ in range(2))
            self.ct = (e3u, e3v, on_device, fill, static)
            h.set_cell_thickness(e3u, e3v, on_device, fill)
        elif op == 'ct_missing':
            self.ct_missing = self._marker()
            h.call('set_cell_thickness_missing_value', self._nan(self.ct_missing))
        elif op == 'ct_clear':                       # NULL: the per-level thickness again, the markers are forgotten
            self.ct, self.ct_missing = None, None
            h.set_cell_thickness(None, None, False, None)
        else:
            raise ValueError(op)
        if op in VERSION_OPS:
            self.version += 1
        elif op != 'transect':
            self.between += 1
        self.log.append(('set', op))

    def set_ct_again(self, h):
        """the cell thickness in the home it has, for the shape, dtype and nt in force"""
        static, on_device = self.ct[4], self.ct[2]
        self.apply(h, ('ct_static_' if static else 'ct_tv_') + ('hbm' if on_device else 'host'))

    def build_weights(self, h):
        if not self.transects:
            self.apply(h, 'transect')
        h.call('build_weights', 16, 360.)
        self.weights_built = True
        self.version += 1

    # ---- computes ----------------------------------------------------------------------------------------------------------
    def draw_compute(self):
        p = numpy.array([KIND_WEIGHTS[k] for k in KINDS])
        if self.uv is not None and self.capturable():
            p[KINDS.index('all')] *= 2.5
        if self.uv is not None and self.sig_state() == 'mismatch':     # the kinds that read the class tracer
            for k in CLASS_KINDS:
                p[KINDS.index(k)] *= 4
        kind = KINDS[self.rng.choice(len(KINDS), p=p / p.sum())]
        form = ['sync', 'async'][self.rng.integers(2)] if kind in BOTH_FORMS else {'all': 'async', 'tracer_all': 'async'}.get(kind, 'sync')
        return kind, form

    def ready(self, h, kind, lazy=None):
        """The setter calls that make `kind` computable.  Always: inputs that exist, borrowed arrays of the (nz, ny, nx) in
        force, a slab inside the steps.  Unless lazy (drawn with probability self.lazy): whatever else a documented refusal
        is pending on -- a tracer, class edges, matching dtype and nt, a static upload of the current shape, no cell thickness
        for the forms that take none, built weights."""
        if lazy is None:
            lazy = kind != 'read' and self.rng.random() < self.lazy
        self.need_uv(h)
        if self.uv[0].shape[1:] != self.shape3():
            self.apply(h, 'uv')
        if self.slab is not None and self.slab[0] >= self.steps() * self.thick.size:
            self.apply(h, 'slab')
        if kind in READS_TRACER:
            s = self.tracer_state()
            if s == 'stale' or (s != 'ok' and not lazy):
                self.apply(h, 'tracer')
        if kind in CLASS_KINDS:
            s = self.sig_state()
            if s == 'stale' or (s == 'mismatch' and not lazy):
                self.apply(h, 'sig')
            if self.edges is None and not lazy:
                self.apply(h, 'edges')
        if kind in NO_CELL_THICK and self.ct is not None and not lazy:
            self.apply(h, 'ct_clear')
        if kind in READS_CELL_THICK:
            s = self.ct_state()
            if s == 'stale' or (s in ('mismatch', 'owned_stale') and not lazy):
                self.set_ct_again(h)
        if not self.weights_built and (kind in NEEDS_NO_WEIGHTS or not lazy):
            self.build_weights(h)

    def causes(self, kind):
        """the documented refusals that hold for `kind` in the present state; none: the call must succeed"""
        c = []
        if kind in READS_TRACER and self.tracer is None:
            c.append('no_tracer')
        if kind in CLASS_KINDS and self.edges is None:
            c.append('no_edges')
        if kind not in NEEDS_NO_WEIGHTS and not self.weights_built:
            c.append('no_weights')
        if kind in NO_CELL_THICK and self.ct is not None:
            c.append('ct_set')
        if kind in READS_TRACER and self.tracer_state() == 'mismatch':
            c.append('tracer_mismatch')
        if kind in CLASS_KINDS and self.sig_state() == 'mismatch':
            c.append('sig_mismatch')
        if kind in READS_CELL_THICK and self.ct_mismatch():
            c.append('ct_mismatch')
        if kind in READS_CELL_THICK and self.ct_state() == 'owned_stale':
            c.append('ct_stale')
        return c

    def capturable(self):
        """nf_field_compute_all_async captures its pass and replays it: a non-null stream, uo / vo resident, the cell thickness
        (when there is one) resident -- a static host array is, once uploaded -- and not the all-steps-in-one-launch form,
        which small grids take with resident uo / vo, two steps or more and no cell thickness"""
        if self.stream == 0 or not self.uv[2]:
            return False
        if self.ct is None:
            return self.steps() == 1
        return self.ct[2] or self.ct[4]

    def owned_steps(self):
        nz = self.thick.size
        if self.slab is None:
            return list(range(self.steps()))
        return [t for t in range(self.steps()) if t * nz < self.slab[1] and (t + 1) * nz > self.slab[0]]

    def owned_levels(self, t):
        """boolean (nz,): the levels of step t inside the slab range"""
        nz = self.thick.size
        s = numpy.arange(t * nz, (t + 1) * nz)
        return numpy.ones(nz, bool) if self.slab is None else (s >= self.slab[0]) & (s < self.slab[1])

    def plan(self, kind, form):
        """what the compute that follows must give: codes == () means "the rows of fresh()", else one of these codes.
        on_fresh: the fresh handle can be brought into the refusing state too (a setter refuses a mismatching array, so it
        cannot when the refusal comes from one)."""
        causes = self.causes(kind)
        unsettled = [s for s in (self.tracer_state(), self.sig_state(), self.ct_state()) if s not in ('none', 'ok')]
        plan = dict(kind=kind, form=form, t=int(self.rng.choice(self.owned_steps())), causes=tuple(causes),
                    codes=tuple(sorted({CODES[c] for c in causes})), on_fresh=bool(causes) and not unsettled,
                    dtype=self.uv[0].dtype.name, uv_on_device=self.uv[2], stream=self.stream, ct_home=self.ct_home(),
                    tracer_set_after_all=self.tracer_set_after_all, capturable=False, replay_after_others=False)
        if kind == 'all' and not causes:
            self.all_seen, self.tracer_set_after_all = True, False
            if self.capturable():
                # the same version gives the same (nt, row_length): the handle passes the same rows tensor again
                plan.update(capturable=True, replay_after_others=self.captured == self.version and self.between > 0)
                self.captured, self.between = self.version, 0
        elif kind != 'all':
            self.between += 1
        self.log.append(('compute', plan))
        return plan

    def fresh(self, new_handle):
        """a new handle brought to the final state by one fixed order of calls; an array that no longer fits uo/vo is left
        out (its setter would refuse it, and no compute that reads it is expected to succeed)"""
        f = new_handle()
        f.set_stream(self.stream)
        f.set_bounds(*self.grid)
        f.set_thickness(self.thick)
        f.set_uv(*self.uv)
        if self.missing is not None:
            f.call('set_missing_value', self.missing)
        if self.sverdrup:
            f.call('set_sverdrup', 1)
        if self.compact:
            f.call('set_compact', 1)
        if self.slab is not None:
            f.call('set_slab_range', *self.slab)
        if self.tracer_state() == 'ok':
            f.set_tracer(*self.tracer)
        if self.tracer_missing is not None:
            f.call('set_tracer_missing_value', self.tracer_missing)
        f.call('set_tracer_reference', self.tracer_ref)
        f.call('set_tracer_wrap', self.tracer_wrap)
        if self.sig_state() == 'ok':
            f.set_class_tracer(*self.sig)
        if self.sig_missing is not None:
            f.call('set_class_tracer_missing_value', self.sig_missing)
        if self.edges is not None:
            f.set_class_edges(self.edges)
        if self.ct_state() == 'ok':
            f.set_cell_thickness(*self.ct[:4])
        if self.ct_missing is not None:
            f.call('set_cell_thickness_missing_value', self.ct_missing)
        for p in self.transects:
            f.add_transect(p)
        if self.weights_built:
            f.call('build_weights', 16, 360.)
        return f


def run_sequence(model, h, nops, compute):
    """nops random ops on handle h; compute(plan) is called for every compute op, after ready() and plan()"""
    for _ in range(nops):
        op = model.draw_op()
        if op == 'compute':
            kind, form = model.draw_compute()
            model.ready(h, kind)
            compute(model.plan(kind, form))
        else:
            model.apply(h, op)


class RecordingHandle:
    """a handle that only writes down what it is asked to do: [(method, args)]"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name, args))
        return record
