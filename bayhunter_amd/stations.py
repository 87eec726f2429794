"""Many stations in one chain pool: chains that share everything but the observed data.

The reference is run station by station (or node by node of a set of dispersion maps): the same periods, priors
and `initparams`, 5-40 chains each, differing in `obsdata.y` and `obsdata.yerr` only.  One after the other these are
small pools, each bound by the latency of a device call; together they are the large batch
the kernels were built for.  The host side of the sampler never sees observed data and the forward kernels do not
either: only the likelihood does, and it subtracts the row of the station a proposal's chain belongs to
(bh_likelihood_sets, bh_eval_set_observations).  A model's forward row and likelihood do not depend on the batch
it is in, so a station's chains are bit for bit the chains of a `ChainPool` of that station alone.

    pool = StationPool({'ST1': joint1, 'ST2': joint2, ...}, initparams, priors, chains_per_station=8,
                       random_seeds=[11, 12, ...]).run()
    pool.station('ST2').posterior()          # the interface of a ChainPool, restricted to the station's chains
    pool.posterior().mean                    # every station's posterior in one pass: [nstations, depths]
    pool.datafits().mean[0]                  # ... and its modelled data, per target: [nstations, samples]
    pool.save()                              # one directory per station, each what a single-station pool writes

One plugin parameter may differ between stations when the pool is told so: the ray parameter `p` of a receiver
function, which in a real network is the mean slowness of the events stacked at each station.

    StationPool(stations, ..., per_station=('p',))     # every station's RFminiModRF keeps its own modelparams['p']

The receiver-function kernel then takes each row's slowness from a table indexed by the row's station
(bh_rf_batch_sets, bh_eval_set_rf_slowness) -- the index the likelihood already uses -- and a row is bit for bit
what the uniform kernel computes at that `p`, so the sentence above about a station's chains still holds.

Everything else stays per pool.  A per-station `gauss` would need a frequency table and a count of active
frequencies per set in the receiver-function kernel, per-station `nsv` or time axes per-row launch constants,
per-station periods per-row descriptors in the dispersion kernels, per-station priors per-chain configurations in
the sampler: all of these are refused.
"""
import inspect
import os

import numpy as np

from . import _lib
from .chains import DEFAULT_INITPARAMS, DEFAULT_PRIORS, ChainPool, GpuEvaluator, CallEvaluator, noise_priors

_COV_NAMES = {_lib.COV_NOCORR: 'NOCORR (no yerr)', _lib.COV_NOCORR_SCALED: 'NOCORR_SCALED (yerr given)',
              _lib.COV_EXP: 'EXP', _lib.COV_GAUSS: 'GAUSS'}


def _plugin_params(target):
    p = target.moddata.plugin
    return type(p).__name__, dict(getattr(p, 'modelparams', None) or {})


PER_STATION = ('p',)         # plugin parameters of receiver-function targets that StationPool(per_station=...) takes


def check_per_station(per_station):
    """-> tuple of the names; ValueError for anything but the supported ones."""
    if isinstance(per_station, str):
        per_station = (per_station,)
    per_station = tuple(per_station or ())
    for key in per_station:
        if key not in PER_STATION:
            raise ValueError("per_station=%r: only %s of a receiver-function target may differ between stations (gauss, nsv, "
                             "time axes and periods are per pool)" % (key, ', '.join(repr(k) for k in PER_STATION)))
    return per_station


def check_stations(names, joints, per_station=()):
    """All stations share the row layout (targets, their order, x axes, plugin parameters) and the covariance model
    of each target (after set_target_covariance): ValueError naming the station and the property otherwise.
    per_station: plugin parameters (of PER_STATION) that the receiver-function targets need not share."""
    per_station = check_per_station(per_station)
    first, name0 = joints[0], names[0]
    for name, joint in zip(names[1:], joints[1:]):
        who = "station %r differs from station %r: " % (name, name0)
        if joint.ntargets != first.ntargets:
            raise ValueError(who + "number of targets (%d, %d)" % (joint.ntargets, first.ntargets))
        if bool(joint.use_mfma) != bool(first.use_mfma):
            raise ValueError(who + "use_mfma")
        for t, (a, b) in enumerate(zip(joint.targets, first.targets)):
            what = who + "target %d " % t
            if a.ref != b.ref or a.noiseref != b.noiseref:
                raise ValueError(what + "ref (%r, %r)" % (a.ref, b.ref))
            ax, bx = np.asarray(a.obsdata.x), np.asarray(b.obsdata.x)
            if ax.shape != bx.shape or not np.array_equal(ax, bx):
                raise ValueError(what + "(%s) x axis (periods / times); per-station axes are not supported" % a.ref)
            if np.asarray(a.obsdata.y).shape != ax.shape:
                raise ValueError(what + "(%s) y does not have the length of x" % a.ref)
            (acls, apar), (bcls, bpar) = _plugin_params(a), _plugin_params(b)
            if acls != bcls:
                raise ValueError(what + "(%s) forward plugin (%s, %s)" % (a.ref, acls, bcls))
            for key in sorted(set(apar) | set(bpar)):
                if key in per_station and a.noiseref == 'rf' and key in apar and key in bpar:
                    continue
                if key not in apar or key not in bpar or apar[key] != bpar[key]:
                    raise ValueError(what + "(%s) plugin parameter %r (%r, %r); per-station plugin parameters are "
                                     "not supported" % (a.ref, key, apar.get(key), bpar.get(key)))
            if a.covmodel != b.covmodel:
                raise ValueError(what + "(%s) covariance model (%s, %s): yerr must be usable at every station or at "
                                 "none" % (a.ref, _COV_NAMES[a.covmodel], _COV_NAMES[b.covmodel]))
            if a.covmodel == _lib.COV_GAUSS and (
                    not np.array_equal(a.valuation.corr_inv, b.valuation.corr_inv)
                    or a.valuation.logcorr_det != b.valuation.logcorr_det):
                raise ValueError(what + "(%s) fixed noise correlation matrix" % a.ref)


MISSING = ('refuse', 'mask')


def find_gaps(names, joints, missing='refuse'):
    """The samples every station lacks, after set_target_covariance: a non-finite obsdata.y, or a non-finite yerr on a
    target that uses it (the yerr-scaled covariance model).  'refuse': ValueError naming station, target and the
    first such sample.  'mask': they become the station's gaps (SingleTarget.present; None for a target without
    any); ValueError naming station and target for a gap in a target with the dense Gaussian model (its R^-1 belongs
    to one n and to contiguous samples) and for a target without a sample left.  -> number of missing samples."""
    if missing not in MISSING:
        raise ValueError("missing=%r: 'refuse' or 'mask'" % (missing,))
    total = 0
    for name, joint in zip(names, joints):
        for t, tg in enumerate(joint.targets):
            ybad = ~np.isfinite(np.asarray(tg.obsdata.y, dtype=np.float64))
            bad = ybad
            if tg.covmodel == _lib.COV_NOCORR_SCALED:
                bad = ybad | ~np.isfinite(np.asarray(tg.obsdata.yerr, dtype=np.float64))
            tg.present = None
            if not bad.any():
                continue
            who = "station %r, target %d (%s): " % (name, t, tg.ref)
            if missing == 'refuse':
                i = int(np.argmax(bad))
                raise ValueError(who + "%s is not finite at sample %d (x = %g); StationPool(missing='mask') treats such "
                                 "samples as gaps of the station" % ('y' if ybad[i] else 'yerr', i, np.asarray(tg.obsdata.x)[i]))
            if tg.covmodel == _lib.COV_GAUSS:
                raise ValueError(who + "%d samples are missing, but a target with the dense Gaussian covariance model "
                                 "cannot have gaps (its fixed R^-1 belongs to one n and to contiguous samples)" % bad.sum())
            if bad.all():
                raise ValueError(who + "no sample is left; stations that lack a whole target are not supported")
            tg.present = ~bad
            total += int(bad.sum())
        joint._batch = None
    return total


def observation_tables(joints, present=False):
    """yobs[nsets, row], set_scale[nsets, row], set_logdet[nsets, ntargets] of stations that passed check_stations, from
    each station's own batch_layout() (so every number is the one a single-station plan uploads); the two tables of
    the yerr-scaled targets are None when no target has that covariance model.  Data gaps (find_gaps): the scaled
    errors and their log-product are taken over a station's kept samples and yobs holds a finite placeholder at a
    gap; present=True appends present[nsets, row] (uint8, 0 at a gap), or None when no station has one."""
    yobs, scale, logdet, have = [], [], [], []
    for joint in joints:                    # one layout at a time: each carries its dense R^-1 (323 KB at n = 201)
        bl = joint.batch_layout(ell=True)
        desc, row = bl['desc'], bl['layout'].row
        yobs.append(bl['yobs'])
        have.append(bl['present'])
        sc, ld = np.ones(row), np.zeros(len(desc))
        for t in range(len(desc)):
            if desc[t].cov == _lib.COV_NOCORR_SCALED:
                d = desc[t]
                sc[d.off:d.off + d.n] = bl['aux'][d.aux_off:d.aux_off + d.n]
                ld[t] = d.logdet_extra
        scale.append(sc)
        logdet.append(ld)
    tabs = (np.stack(yobs), np.stack(scale), np.stack(logdet))
    if not any(d.cov == _lib.COV_NOCORR_SCALED for d in desc):
        tabs = (tabs[0], None, None)
    have = np.stack(have)
    return tabs + ((None if have.all() else have),) if present else tabs


def rf_slowness_table(joints):
    """p[nstations, nrf]: modelparams['p'] of every station's own receiver-function plugins, in the order of the row
    layout's receiver functions (JointTarget.batch_layout)."""
    from .plugins import RFminiModRF
    return np.array([[float(t.moddata.plugin.modelparams['p']) for t in joint.targets
                      if isinstance(t.moddata.plugin, RFminiModRF)] for joint in joints], dtype=np.float64)


class StationGpuEvaluator(GpuEvaluator):
    """GpuEvaluator whose evaluation plans carry one observation set per station: a plan is built from the first
    station's layout and given every station's observed data and the station of each of its group's chains -- and,
    with per_station=('p',), every station's ray parameters."""
    per_chain = True

    def __init__(self, joints, station_of_chain, device=None, per_station=()):
        GpuEvaluator.__init__(self, joints[0], device)
        self.joints, self.station_of_chain = list(joints), np.asarray(station_of_chain, dtype=np.int32)
        self.per_station = check_per_station(per_station)
        self._tables = None

    def buffers(self, rows, Lmax, ntargets, chains):
        if self._tables is None:            # (after the pool has chosen the covariance models)
            self._tables = observation_tables(self.joints, present=True)
        packed, nlay, noise, chain = GpuEvaluator.buffers(self, rows, Lmax, ntargets)
        yobs, scale, logdet, present = self._tables
        plan = self._plans[packed.ctypes.data]
        plan.set_observations(yobs, self.station_of_chain[chains[0]:chains[1]], scale, logdet)
        if present is not None:
            plan.set_gaps(present)
        if 'p' in self.per_station and plan.nrf:
            plan.set_rf_slowness(rf_slowness_table(self.joints))
        return packed, nlay, noise, chain


class StationCallEvaluator(CallEvaluator):
    """Adapter for a plain function (packed, nlay, noise, station[B]) -> (logL, misfits)."""

    def __init__(self, fn, station_of_chain):
        CallEvaluator.__init__(self, fn)
        self.station_of_chain = np.asarray(station_of_chain, dtype=np.int32)

    def submit(self, group, packed, nlay, noise):
        n = packed.shape[0]
        return self.fn(packed, nlay, noise, self.station_of_chain[group.first + group.chain[:n]])


def _takes_station(fn):
    try:
        params = [p for p in inspect.signature(fn).parameters.values()
                  if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
    except (TypeError, ValueError):
        return False
    return len(params) >= 4


class StationView(ChainPool):
    """The chains of one station of a StationPool behind the interface of a ChainPool (`models, misfits, likes,
    noise, vpvs, iter, nchains, first, counters(), chain(i), weighted(i), final(), outliers(), posterior(),
    datafits(), moho(), interfaces(), scalars(), convergence(), depth_covariance(), data_covariance(), sensitivity(), save()`, `targets`, `priors`,
    `initparams`): views of the pool's arrays, chains numbered from 0."""

    def __init__(self, pool, s):
        inner, c = pool.pool, pool.chains_per_station
        self._parent, self._range = inner, slice(s * c, (s + 1) * c)
        self.lib, self.targets, self.priors = inner.lib, pool.stations[s], inner.priors
        self.initparams = dict(inner.initparams, nchains=c, station=pool.names[s],
                               savepath=os.path.join(inner.initparams['savepath'], str(pool.names[s])))
        self.nchains = self.nchains_total = c
        self.first = 0
        self.ntargets, self.cfg = inner.ntargets, inner.cfg
        self.iter_burnin, self.iter_main, self.iterations = inner.iter_burnin, inner.iter_main, inner.iterations
        self.maxlayers, self.Lmax, self.nmodels = inner.maxlayers, inner.Lmax, inner.nmodels
        self.seeds = inner.seeds[self._range]
        for name in ('models', 'misfits', 'likes', 'noise', 'vpvs', 'iter'):
            setattr(self, name, getattr(inner, name)[self._range])
        self.groups = ()
        self._closed_counters = self._closed_advance = None

    def counters(self):
        return tuple(a[self._range] for a in self._parent.counters())

    def run(self, progress=None):
        raise _lib.BayHunterAmdError("a station's chains run with their pool: StationPool.run()")

    def advance(self):
        raise _lib.BayHunterAmdError("device calls are counted for the whole pool: StationPool.advance()")


class StationPool(object):
    """`StationPool(stations, initparams, modelpriors, chains_per_station=..., random_seeds=...)`: ONE lock-step pool
    of nstations * chains_per_station chains; chain s * chains_per_station + i is chain i of station s.

    stations            sequence of JointTargets, or an ordered mapping name -> JointTarget (names default to
                        'st000', 'st001', ...; they name the directories save() writes).  All share targets, x axes,
                        plugin parameters and -- with the pool's priors -- the covariance model of every target;
                        they differ in obsdata.y and obsdata.yerr.  Anything else: ValueError naming station and property.
    chains_per_station  default initparams['nchains']
    random_seeds        one per station: station s gets exactly the chain seeds of
                        ChainPool(random_seed=random_seeds[s], nchains=chains_per_station), so a station's chains do
                        not depend on which other stations share the pool.  A single number or None: every station
                        draws from the next values of RandomState(random_seeds).
    seeds               [nstations][chains_per_station] explicit chain seeds instead
    evaluator           None: the GPU (one evaluation plan per chain group, carrying every station's observations);
                        a function (packed, nlay, noise, station[B]) -> (logL, misfits); a function of three
                        arguments or an object with buffers/submit/collect is passed to ChainPool as it is
    per_station         () or ('p',): plugin parameters of the receiver-function targets that every station keeps
                        for itself (the ray parameter; module docstring).  Without it stations that differ in `p`
                        are refused like any other difference; any other name: ValueError listing what is supported.
                        CPU evaluators get each row's station and use that station's own plugin as they always did
    missing             'refuse' (default): a non-finite obsdata.y, or a non-finite yerr on a target that uses it, is a
                        ValueError naming station, target and sample.  'mask': those samples are the station's GAPS -- a
                        map node without long periods, a period that failed quality control.  Every row is still
                        modelled on the pool's axis; the likelihood leaves out what the row's station lacks and values
                        the target as the reference values it when those lines have been deleted from the data file
                        (n' kept samples: rms, 2 n' log sigma, n' log 2 pi; scaled_err = yerr / min over the kept
                        samples; the exponential law on the compacted vector, kept neighbours being neighbours).
                        Refused: a gap in a target with the dense Gaussian model, and a target without a sample left.
                        Two consequences of modelling on the pool's axis: (1) a kept value is not bit for bit what a
                        run on the shortened axis gives -- the root search of period k starts from the root of period
                        k - 1, so the two differ at its stopping tolerance, 1e-6 relative; (2) a model whose
                        dispersion search fails at a period the station does not use still fails for that station.
                        (A yerr with a NaN is dropped as a whole by ObservedData, as in the reference: give a gap any
                        positive yerr, or inf.)  station(s).datafits() reports the observed value and the residual of
                        a gap as NaN; CPU evaluators find the gaps in SingleTarget.present, which JointTarget.evaluate
                        honours
    groups, nthreads, nmodels, lookahead   as for ChainPool
    shard               not supported yet (stations would have to be sharded whole): ValueError

    `pool.pool` is the ChainPool of all chains; `station(s)` (index or name) a StationView."""

    def __init__(self, stations, initparams=None, modelpriors=None, chains_per_station=None, random_seeds=None,
                 seeds=None, evaluator=None, groups=None, nthreads=None, shard=None, nmodels=None, lookahead=None,
                 device=None, per_station=(), missing='refuse'):
        self.per_station = check_per_station(per_station)
        if missing not in MISSING:
            raise ValueError("missing=%r: 'refuse' or 'mask'" % (missing,))
        self.missing = missing
        if shard is not None:
            raise ValueError("StationPool does not take shard=(rank, world) yet: give every rank a StationPool of its "
                             "own stations")
        if hasattr(stations, 'keys'):
            self.names, self.stations = [k for k in stations.keys()], [stations[k] for k in stations.keys()]
        else:
            self.stations = list(stations)
            self.names = ['st%03d' % s for s in range(len(self.stations))]
        if not self.stations:
            raise ValueError("no station")
        if len(set(self.names)) != len(self.names):
            raise ValueError("station names must be unique")
        S = self.nstations = len(self.stations)
        ip = dict(initparams or {})
        if seeds is not None:
            seeds = np.asarray(seeds)
            if seeds.ndim != 2 or seeds.shape[0] != S:
                raise ValueError("seeds: [nstations][chains_per_station]")
            if chains_per_station is not None and int(chains_per_station) != seeds.shape[1]:
                raise ValueError("seeds: [nstations][chains_per_station]")
            chains_per_station = seeds.shape[1]
        if chains_per_station is None:
            chains_per_station = ip.get('nchains', DEFAULT_INITPARAMS['nchains'])
        c = self.chains_per_station = int(chains_per_station)
        if c < 1:
            raise ValueError("chains_per_station < 1")
        if seeds is None:
            if random_seeds is None or np.ndim(random_seeds) == 0:
                rstate = np.random.RandomState(random_seeds)
                seeds = [[rstate.randint(1000) for _ in range(c)] for _ in range(S)]
            else:
                if len(random_seeds) != S:
                    raise ValueError("random_seeds: one per station")
                seeds = []
                for rs in random_seeds:             # ChainPool's own draw (src/mcmcOptimizer.py:133-137)
                    rstate = np.random.RandomState(rs)
                    seeds.append([rstate.randint(1000) for _ in range(c)])
            seeds = np.asarray(seeds)
        self.station_of_chain = np.repeat(np.arange(S, dtype=np.int32), c)
        # the covariance model of every station's targets, chosen like ChainPool chooses the first station's
        priors = dict(DEFAULT_PRIORS)
        priors.update(modelpriors or {})
        first = self.stations[0]
        for name, joint in zip(self.names, self.stations):
            if joint.ntargets != first.ntargets:
                raise ValueError("station %r differs from station %r: number of targets (%d, %d)"
                                 % (name, self.names[0], joint.ntargets, first.ntargets))
        np_ = noise_priors(priors, first.targets)
        corrfix, corr = [bool(p[0][0]) for p in np_], [p[0][1] for p in np_]
        rcond = ip.get('rcond', DEFAULT_INITPARAMS['rcond'])
        for joint in self.stations[1:]:
            joint.set_target_covariance(corrfix, corr, rcond)
        first.set_target_covariance(corrfix, corr, rcond)
        check_stations(self.names, self.stations, self.per_station)
        self.ngaps = find_gaps(self.names, self.stations, missing)
        if evaluator is None:
            evaluator = StationGpuEvaluator(self.stations, self.station_of_chain, device, self.per_station)
        elif not hasattr(evaluator, 'submit') and _takes_station(evaluator):
            evaluator = StationCallEvaluator(evaluator, self.station_of_chain)
        self.pool = ChainPool(first, initparams=ip, modelpriors=modelpriors, nchains=S * c, seeds=seeds.reshape(-1),
                              evaluator=evaluator, groups=groups, nthreads=nthreads, nmodels=nmodels,
                              lookahead=lookahead)
        self.evaluator = self.pool.evaluator

    # -- the pool of all chains -----------------------------------------------------------------
    def run(self, progress=None):
        self.pool.run(progress)
        return self

    def close(self):
        self.pool.close()

    @property
    def closed(self):
        return self.pool.closed

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def nchains(self):
        return self.pool.nchains

    @property
    def seconds(self):
        return self.pool.seconds

    @property
    def evaluated(self):
        return self.pool.evaluated

    def advance(self):
        return self.pool.advance()

    def counters(self):
        return self.pool.counters()

    # -- per station ------------------------------------------------------------------------------
    def station(self, s):
        """The chains of station `s` (index or name) as a ChainPool-like view."""
        if not isinstance(s, (int, np.integer)) or isinstance(s, bool):
            if s not in self.names:
                raise KeyError("no station %r" % (s,))
            s = self.names.index(s)
        if not 0 <= s < self.nstations:
            raise IndexError("station %d of %d" % (s, self.nstations))
        return StationView(self, int(s))

    def posterior(self, dep_int=None, depint=1, dev=0.05, exclude_outliers=True, selection='weighted', device=None,
                  strict=True):
        """The velocity-depth posterior of every station in one pass over the pool's rows (posterior.summarize_sets):
        per station, selection and outlier chains as station(s).posterior(...) takes them, and the very dict it
        returns ('chains' numbered within the station).  -> posterior.StationPosterior: `stations[name]` those
        dicts, `failed` {name: message} for stations without a posterior (no main-phase rows left, all Vs within
        0.025 km/s, best chain's median likelihood 0), and the stacked single models `dep`, `mean / median / std /
        vmin / vmax [nstations, D]`, `mode [nstations, D - 1]` with NaN rows for failed stations.  strict=True: a
        failed station is a ValueError naming the first one."""
        from .posterior import stations_posterior
        return stations_posterior(self, dep_int, depint, dev, exclude_outliers, selection, device, strict)

    def datafits(self, selection='weighted', dev=0.05, exclude_outliers=True, q=(2.5, 16, 50, 84, 97.5), nbins=100,
                 device=None, strict=True, max_rows=None):
        """The statistics of the modelled data of every station in one pass (datafits.summarize_sets): one forward
        pass over the rows posterior() takes -- every row at its own station's ray parameter with per_station=('p',)
        -- and one segmented reduction (bh_datafits_sets_*), instead of a forward pass and a handle per station.  Per
        station the very dict station(s).datafits(...) returns, bit for bit ('chains' and 'bestfits' numbered within
        the station; the observed value and the residual of a gap NaN).  -> datafits.StationDatafits: `stations[name]`
        those dicts, `failed` {name: message}, and per target the stacked `mean / std / median / min / max / best /
        residual [nstations, S]`, `quantiles [nstations, len(q), S]`, and `nmodels`, `nexcluded [nstations]`, with NaN
        rows for failed stations.  strict=True: a failed station is a ValueError naming the first one.  max_rows: the
        stations are taken in runs of whole stations of at most that many rows (default: what half of the free device
        memory holds); no result depends on it."""
        from .datafits import stations_datafits
        return stations_datafits(self, selection, dev, exclude_outliers, q, nbins, device, strict, max_rows)

    def moho(self, moho=None, mohovs=4.2, selection='weighted', dev=0.05, exclude_outliers=True, nbins=50, device=None,
             tradeoff=False):
        """Moho depth +- std, crustal Vs and the share of models with a Moho of every station in one pass over the
        pool's rows (moho.summarize_sets: one launch derives every row, one reduces all stations): per station the
        numbers station(s).moho(...) reports.  -> moho.StationMoho: `names`, `moho / vs_crust / vs_last / vs_jump`
        = dict(median, mean, std, min, max [nstations]), `nmodels`, `nexcluded`, `fraction [nstations]`, `hist
        [nstations, nbins]` of the Moho depth over the shared `edges`, `failed` {name: message}.  A station without a
        model that has a Moho is a hole of the map (NaN, nmodels 0), not an error.
        tradeoff=True adds `tradeoff` = {vs_last, vs_crust, vs_jump: dict(counts [nstations, nbins, nbins], xedges,
        yedges [nstations, nbins + 1], mode [nstations, 2])}: per station the three joint histograms against the Moho
        depth that station(s).moho()['tradeoff'] holds, bit for bit, over the station's own edges, from one more
        launch (bh_hist2d_sets; nbins <= 64); NaN edges and mode for a hole of the map."""
        from .moho import stations_moho
        return stations_moho(self, moho, mohovs, selection, dev, exclude_outliers, nbins, device, tradeoff)

    def interfaces(self, dep_edges=None, jump_edges=None, selection='weighted', dev=0.05, exclude_outliers=True,
                   device=None):
        """The discontinuity section of the network in one pass over the pool's rows (interfaces.summarize_sets): per
        station and depth bin the probability of an interface, of a negative and of a positive one, and the Vs jump,
        over edges all stations share.  -> interfaces.StationInterfaces: `names`, `stations` {name: the dict
        station(s).interfaces(...) returns, field for field}, `p_interface / p_neg / p_pos / jump_mean / count
        [nstations, depth bins]` (a station without a model is a row of NaN), `dep_edges`, `jump_edges`, `failed`
        {name: message}."""
        from .interfaces import stations_interfaces
        return stations_interfaces(self, dep_edges, jump_edges, selection, dev, exclude_outliers, device)

    def scalars(self, selection='weighted', dev=0.05, exclude_outliers=True, nbins=20, pairs=(), pair_bins=50, moho=None,
                mohovs=4.2, device=None, strict=False, max_rows=None):
        """The posterior of the sampler's scalar parameters of every station in one pass over the pool's rows
        (scalars.summarize_sets: one segmented reduction and one bh_hist2d_sets launch for all stations): "the sigma of
        the receiver-function noise at every station", "the crustal Vp/Vs map".  Arguments as station(s).scalars(...);
        per station every field is bit for bit what that returns ('chains' numbered within the station).
        -> scalars.StationScalars: `names`, `stations[name]` those dicts, `failed` {name: message}, `columns`,
        `nmodels / nexcluded [nstations]`, `stats[column]` = dict(median, mean, std, min, max, mode, constant
        [nstations], hist [nstations, nbins], edges [nstations, nbins + 1]), `pairs[(x, y)]` = dict(counts [nstations,
        pair_bins, pair_bins], xedges, yedges, mode [nstations, 2]); NaN for a failed station or one without rows.
        strict=True: such a station is a ValueError naming the first one.  max_rows: the stations are taken in runs of
        whole stations of at most that many rows (default: what half of the free device memory holds); no result
        depends on it."""
        from .scalars import stations_scalars
        return stations_scalars(self, selection, dev, exclude_outliers, nbins, pairs, pair_bins, moho, mohovs, device,
                                strict, max_rows)

    def convergence(self, nlags=1024, depths=(), dev=0.05, exclude_outliers=True, rhat_max=1.01, ess_min=None,
                    device=None, strict=True, max_rows=None):
        """Which stations have converged: split R-hat and the effective sample size of every station in one pass
        (convergence.py): every station a group of half chains, one segmented reduction and one bh_autocov_sets launch
        per run of whole stations.  Arguments as station(s).convergence(...); per station every field is bit for bit
        what that returns.  -> convergence.StationConvergence: `names`, `stations[name]` those dicts, `failed` {name:
        message}, `columns`, `rhat / ess / tau / truncated / converged` {column: [nstations]} (NaN for a failed station)
        and `window [nstations, 2]`.  strict=True: a failed station is a ValueError naming the first one.  max_rows: runs
        of whole stations of at most that many entries; no result depends on it."""
        from .convergence import stations_convergence
        return stations_convergence(self, nlags, depths, dev, exclude_outliers, rhat_max, ess_min, device, strict,
                                    max_rows)

    def depth_covariance(self, dep_int=None, extras=('vpvs',), selection='weighted', dev=0.05, exclude_outliers=True,
                         device=None, strict=True, max_rows=None, budget_bytes=1 << 30):
        """The posterior covariance and correlation matrix of the Vs(z) profile of every station in one pass
        (covariance.summarize_sets: one segmented scan for the means and one bh_depthcov_sets call per run of stations).
        Arguments as station(s).depth_covariance(...); per station every field is bit for bit what that returns ('chains'
        numbered within the station).  -> covariance.StationDepthCovariance: `names`, `stations[name]` those dicts,
        `failed` {name: message}, `columns` ('vs@<z>' per depth, then the extras), `dep`, the stacked `cov / corr
        [nstations, K, K]`, `mean / std [nstations, K]`, `nmodels [nstations]`; NaN for a failed station.  strict=True: a
        failed station is a ValueError naming the first one.  max_rows: runs of whole stations of at most that many rows
        (default: what half of the free device memory holds); budget_bytes: bound on the S matrices of one call (1 GiB;
        1 024 stations of 201 depths are 331 MB).  No result depends on either."""
        from .covariance import stations_depth_covariance
        return stations_depth_covariance(self, dep_int, extras, selection, dev, exclude_outliers, device, strict, max_rows,
                                         budget_bytes)

    def data_covariance(self, dep_int=None, extras=('vpvs',), selection='weighted', dev=0.05, exclude_outliers=True,
                        device=None, strict=True, max_rows=None):
        """The posterior cross-covariance and correlation of the Vs(z) profile and the modelled data of every station in
        one pass (datacov.summarize_sets: one forward pass -- every row at its own station's ray parameter with
        per_station=('p',) -- two segmented scans for the centres and one bh_datacov_sets call per run of stations).
        Arguments as station(s).data_covariance(...); per station every field is bit for bit what that returns ('chains'
        numbered within the station).  -> datacov.StationDataCovariance: `names`, `stations[name]` those dicts, `failed`
        {name: message}, `columns` ('vs@<z>' per depth, then the extras), `dep`, `targets`, `x`, the stacked `cov / corr
        [nstations, K, S]`, `mean_x / std_x [nstations, K]`, `mean_y / std_y [nstations, S]`, `nmodels / nexcluded
        [nstations]`; NaN for a failed station.  strict=True: a failed station is a ValueError naming the first one.
        max_rows: runs of whole stations of at most that many rows (default: what half of the free device memory holds);
        no result depends on it."""
        from .datacov import stations_data_covariance
        return stations_data_covariance(self, dep_int, extras, selection, dev, exclude_outliers, device, strict, max_rows)

    def sensitivity(self, ref=None, dep_edges=None, kind='vs_total', selection='weighted', dev=0.05,
                    exclude_outliers=True, device=None, max_rows=None, strict=False):
        """The posterior mean and spread of the depth-binned phase-velocity sensitivity kernel of every station in one
        pass (sensitivity.summarize_sets: per run of rows the search, the pass and bh_sens_sets_add on one handle).
        Arguments as station(s).sensitivity(...); per station every field is bit for bit what that returns ('chains'
        numbered within the station).  -> sensitivity.StationSensitivity: `names`, `stations[name]` those dicts,
        `failed` {name: message}, `ref`, `periods`, `edges`, `kind`, the stacked `mean / std / min / max [nstations,
        nper, bins]`, `halfspace_mean / halfspace_std / nmodels / nexcluded [nstations, nper]`; NaN for a failed
        station.  strict=True: a failed station is a ValueError naming the first one.  max_rows: runs of whole stations
        of at most that many rows, a larger station in whole blocks (default: what half of the free device memory
        holds); no result depends on it."""
        from .sensitivity import stations_sensitivity
        return stations_sensitivity(self, ref, dep_edges, kind, selection, dev, exclude_outliers, device, max_rows, strict)

    def group_sensitivity(self, ref=None, dep_edges=None, kind='vs_total', selection='weighted', dev=0.05,
                          exclude_outliers=True, device=None, max_rows=None, strict=False):
        """sensitivity() for the group velocity (ChainPool.group_sensitivity): every station's depth-binned dU/dm in one
        pass; per station every field is bit for bit what station(s).group_sensitivity(...) returns.  `ref` defaults to
        the stations' only fundamental-mode group target.  -> sensitivity.StationSensitivity with `velocity` 'group'."""
        from .sensitivity import stations_sensitivity
        return stations_sensitivity(self, ref, dep_edges, kind, selection, dev, exclude_outliers, device, max_rows, strict,
                                    velocity='group')

    def ell_sensitivity(self, ref=None, dep_edges=None, kind='vs_total', selection='weighted', dev=0.05,
                        exclude_outliers=True, device=None, max_rows=None, strict=False):
        """sensitivity() for the Rayleigh-wave ellipticity (ChainPool.ell_sensitivity): every station's depth-binned dE/dm
        in one pass; per station every field is bit for bit what station(s).ell_sensitivity(...) returns.  `ref` defaults
        to the stations' only ellipticity target.  -> sensitivity.StationSensitivity with `velocity` 'ellipticity'."""
        from .sensitivity import stations_sensitivity
        return stations_sensitivity(self, ref, dep_edges, kind, selection, dev, exclude_outliers, device, max_rows, strict,
                                    velocity='ellipticity')

    def rf_sensitivity(self, ref=None, dep_edges=None, kind='vs_total', t=None, every=1, selection='weighted', dev=0.05,
                       exclude_outliers=True, device=None, max_rows=None, strict=False):
        """The depth-binned receiver-function sensitivity kernel of every station in one pass (ChainPool.rf_sensitivity;
        sensitivity.rf_summarize_sets: per run of rows the pass and bh_rf_sens_sets_add on one handle) -- every station at
        its own ray parameter with per_station=('p',).  Per station every field is bit for bit what
        station(s).rf_sensitivity(...) returns.  -> sensitivity.StationRfSensitivity: `names`, `stations[name]` those
        dicts, `failed`, and the stacked arrays [nstations, nsel, bins]."""
        from .sensitivity import stations_rf_sensitivity
        return stations_rf_sensitivity(self, ref, dep_edges, kind, t, every, selection, dev, exclude_outliers, device,
                                       max_rows, strict)

    def save(self, savepath=None):
        """One directory <savepath>/<station name> per station, each holding what a ChainPool of that station alone
        writes (data/c%03d_... numbered from 0, data/<station name>_config.pkl with the station's targets).
        -> number of .npy files written."""
        savepath = savepath or self.pool.initparams['savepath']
        written = 0
        for s, name in enumerate(self.names):
            written += self.station(s).save(os.path.join(savepath, str(name)))
        return written
