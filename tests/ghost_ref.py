"""The path loop's ghosts and roll-backs as a model in plain Python: test infrastructure.

Two parts.  (a) The three-state machine: tests/sweep_ref.sweep_model with its `ghosts=` argument -- alive, ghost, dead; the rules
are csrc/sweep.h:1025-1031 and :670-673 and are stated there.  (b) `trace_model`: csrc/trace.hip:219-418 for ONE label at the
level of its decisions -- which call may make ghosts, what the journal holds, when the label rolls back, to where, and what the
roll-back restores.  Target order, the path search and the exact flood are the oracle's (oracle/__init__.py), the checker of the
whole GPU tier; the loop, the alive bytes (0 dead, 1 alive, 3 ghost), the journal, the saved rail weights and the counters are
this file's own.  Nothing of the product is imported.

What the model returns (a namespace):
  paths     the label's paths, as oracle.pipeline.trace(return_paths=True) returns them
  calls     one record per invalidation call, in the order the loop makes them: path (index of the path), kind ("sweep", "redo" or
            "soma"), cls (sweep_ref.classify of the call on the state it saw; None for a redo), made / killed_ghosts / killed (sorted
            linear indices; a redo or an uncertified call: what the exact flood killed), certified, n_many
  rollbacks one record per roll-back: reason (one of REASONS), at (the path index the loop had reached), to (the path whose call is
            redone), journal (entries revived), rails (path vertices whose weight came back), rail_paths (paths that had such a
            vertex), ghost_calls_since (the calls that made a ghost between `to` and the roll-back)
  counters  what a task record (kh_label_t) carries and this sequence determines:
              n_paths, n_vertices, stat_ghost_calls (calls that made a ghost), stat_rollbacks      always
              stat_sweep_calls   = the calls that are no redo: invalidate.h:71 runs the sweep on every call that is not forced to the
                                   heap, provided the label has levels (nlev != 0, the planner's business: the GPU test asserts it from
                                   the record) and 0 < npath <= min(32 766, voxels) (checked here)
              stat_sweep_bails   = the redone calls (invalidate.h:92-93) + the calls the sweep does not certify: class C (a ninth
                                   candidate), the calls of a path named in `abandon`, and -- where ghosts are not allowed: mode "off", the soma
                                   call -- class M
              stat_sweep_why     = SW_BAIL_M (1) if a call was redone or bailed for class M; the bits of C (2) and of a forced bail are
                                   left to the test (the knob decides the bit)
            NOT derived: stat_sweep_levels and stat_sweep_events (chunk and window bookkeeping of sweep.h, not decisions),
            stat_heap_pushes / stat_settled (the heap emulation and the searches have tests of their own), the cycle counters, and
            last_retries (the planner's scratch sizes).  A fifth candidate needs the spill table, whose size is the planner's: the model
            reports max_n_many and the GPU test requires ev_spill >= it, so that class C is the ninth candidate alone.
  ghosts_at_end   ghosts alive when the loop ended (max_paths can end it with some)

Modes: "ghosts" (the default of the engine), "paranoid" (every call that makes a ghost is rolled back at the top of the next
iteration, trace.hip:240), "no_journal" (the pool refused the journal: the same control flow as paranoid, the log stays in the
first work list, trace.hip:369-375) and "off" (no ghost is ever made: a class-M call is redone by the heap at once).
"""
from types import SimpleNamespace

import numpy as np

import sweep_ref

REASONS = ("ghost target", "valid == 0", "sweep abandoned", "paranoid", "no journal")
MODES = ("ghosts", "paranoid", "no_journal", "off")
SW_BAIL_M = 1


def _locs(path, shape):
    p = np.asarray(path, dtype=np.int64).reshape(-1, 3)
    return p[:, 0] + shape[0] * (p[:, 1] + shape[1] * p[:, 2])


def trace_model(labels, DBF, anisotropy=(1, 1, 1), scale=10, const=10, pdrf_scale=5000, pdrf_exponent=16,
                soma_detection_threshold=1100, soma_acceptance_threshold=4000, soma_invalidation_scale=0.5,
                soma_invalidation_const=0, fix_branching=True, manual_targets_before=None, manual_targets_after=None, root=None,
                max_paths=None, voxel_graph=None, mode="ghosts", abandon=(), soundness=False):
    """One label through the loop.  The arguments of kimimaro.trace.trace, then
    mode       one of MODES
    abandon    indices of the paths whose ball a capacity knob of the planner makes the sweep abandon, every time it is tried
    soundness  after every call assert: certainly dead <= the oracle's dead set <= dead u ghosts (the oracle floods its own exact
               mask with the same paths, call by call)
    """
    import oracle as K
    from oracle import pipeline as P
    assert mode in MODES
    if voxel_graph is not None:
        vcg = np.asfortranarray(voxel_graph, dtype=np.uint32)
        with K.voxel_graph(vcg):
            return _trace_model(K, P, labels, DBF, anisotropy, scale, const, pdrf_scale, pdrf_exponent, soma_detection_threshold,
                                soma_acceptance_threshold, soma_invalidation_scale, soma_invalidation_const, fix_branching,
                                manual_targets_before, manual_targets_after, root, max_paths, vcg, mode, abandon, soundness)
    return _trace_model(K, P, labels, DBF, anisotropy, scale, const, pdrf_scale, pdrf_exponent, soma_detection_threshold,
                        soma_acceptance_threshold, soma_invalidation_scale, soma_invalidation_const, fix_branching,
                        manual_targets_before, manual_targets_after, root, max_paths, None, mode, abandon, soundness)


def _trace_model(K, P, labels, DBF, anisotropy, scale, const, pdrf_scale, pdrf_exponent, soma_detection_threshold,
                 soma_acceptance_threshold, soma_invalidation_scale, soma_invalidation_const, fix_branching, before, after, root,
                 max_paths, vcg, mode, abandon, soundness):
    import scipy.ndimage
    # ---- the preamble, kimimaro/trace.py:96-172 as oracle.pipeline.trace restates it (no decision of the loop lies here)
    before = [tuple(int(v) for v in p) for p in (before or [])]
    after = [tuple(int(v) for v in p) for p in (after or [])]
    dbf_max = np.max(DBF)
    labels = np.asfortranarray(np.asarray(labels) != 0, dtype=np.uint8).copy(order="F")
    DBF = np.asfortranarray(DBF, dtype=np.float32).copy(order="F")
    soma = False
    if dbf_max > soma_detection_threshold:
        filled = scipy.ndimage.binary_fill_holes(labels)
        if int(np.count_nonzero(filled)) > int(np.count_nonzero(labels)):
            labels = np.asfortranarray(filled.astype(np.uint8))
            bb = bool(np.all(labels))
            DBF = K.edt(labels, anisotropy, black_border=bb) if vcg is None else K.edt_graph(labels, vcg, anisotropy, black_border=bb)
        dbf_max = np.max(DBF)
        soma = bool(dbf_max > soma_acceptance_threshold)
    soma_radius = 0.0
    if soma:
        if root is not None:
            before.insert(0, tuple(int(v) for v in root))
        root = P.find_soma_root(DBF, dbf_max)
        soma_radius = dbf_max * soma_invalidation_scale + soma_invalidation_const
    elif root is None:
        root = P.find_root(labels, anisotropy)
    root = tuple(int(v) for v in root)
    shape = labels.shape
    DBF = K.zero2inf(DBF)
    DAF, far = K.euclidean_distance_field(labels, root, anisotropy, DBF[root] if soma else 0)
    DAF = K.inf2zero(DAF)
    order = K.target_order(labels, DAF).astype(np.int64)       # CachedTargetFinder's order: the first alive voxel is the target
    PDRF = K.compute_pdrf(dbf_max, pdrf_scale, pdrf_exponent, DBF, DAF, DAF[far])
    pdrf = PDRF.reshape(-1, order="F")                          # (a view: rails are written through it)
    field_dist = None if fix_branching else K.field_distances(PDRF, root)
    dbf_flat = DBF.reshape(-1, order="F")
    nf = int(np.count_nonzero(labels))

    # ---- the loop's state, trace.hip:138-161
    alive = labels.reshape(-1, order="F").copy()                # 0 dead, 1 alive, 3 ghost (sweep.h:47)
    exact = labels.copy(order="F") if soundness else None       # the oracle's own mask, flooded with the same paths
    exact_done = [-2]                                           # the last path index `exact` has been flooded with
    calls, rollbacks = [], []
    c = dict(n_paths=0, n_vertices=0, stat_ghost_calls=0, stat_rollbacks=0, stat_sweep_calls=0, stat_sweep_bails=0, stat_sweep_why=0)
    max_n_many = [0]
    ghosts_on = mode != "off"
    paranoid, no_journal = mode == "paranoid", mode == "no_journal"
    abandon = frozenset(int(a) for a in abandon)

    def flood(path, sc, cn):
        """the exact flood (the heap emulation's result) on the loop's mask, which holds no ghost then"""
        assert not (alive == 3).any()
        m = alive.reshape(shape, order="F").copy(order="F")     # (the oracle floods in place)
        n, m = K.roll_invalidation_ball_inside_component(m, DBF, sc, cn, anisotropy, path, voxel_connectivity_graph=vcg)
        after_flat = m.reshape(-1, order="F")
        killed = np.flatnonzero((alive != 0) & (after_flat == 0))
        assert killed.size == n
        alive[killed] = 0
        return killed

    def check_sound(k, path, sc, cn):
        if not soundness:
            return
        if exact_done[0] < k:
            K.roll_invalidation_ball_inside_component(exact, DBF, sc, cn, anisotropy, path, voxel_connectivity_graph=vcg)
            exact_done[0] = k
        obj = labels.reshape(-1, order="F") != 0
        ex_dead = set(np.flatnonzero(obj & (exact.reshape(-1, order="F") == 0)).tolist())
        dead = set(np.flatnonzero(obj & (alive == 0)).tolist())
        gh = set(np.flatnonzero(alive == 3).tolist())
        assert dead <= ex_dead, ("call of path %d kills voxels the reference keeps" % k, sorted(dead - ex_dead)[:8])
        assert ex_dead <= dead | gh, ("call of path %d: the reference kills voxels that are neither dead nor ghosts" % k,
                                      sorted(ex_dead - dead - gh)[:8])

    def invalidate(k, path, sc, cn, allow_ghosts, redo, heap_ok, kind):
        """invalidate.h:56-132 for the call of path k.  Returns None when the caller has to roll back (ctl.u0), else
        (killed voxels that were no ghosts, ghosts made, ghosts killed) as index arrays, the mask updated."""
        rec = SimpleNamespace(path=k, kind=kind, cls=None, made=(), killed_ghosts=(), killed=(), certified=False, n_many=0)
        calls.append(rec)
        npath = len(path)
        none = np.zeros(0, np.int64)
        if not redo and 0 < npath <= min(32766, nf):
            c["stat_sweep_calls"] += 1
            res = sweep_ref.sweep_model(alive.reshape(shape, order="F"), anisotropy, path,
                                        sweep_ref.ball_radii(DBF, _locs(path, shape), sc, cn), graph=vcg,
                                        ghosts=np.flatnonzero(alive == 3))
            rec.cls, rec.n_many = sweep_ref.classify(res), res.n_many
            max_n_many[0] = max(max_n_many[0], res.n_many)
            undecided = res.M.size != 0 and not allow_ghosts
            if res.max_cand < 9 and k not in abandon and not undecided:
                rec.certified = True
                rec.made, rec.killed_ghosts = res.made, res.KG
                rec.killed = np.setdiff1d(res.D, res.KG)
                alive[res.D] = 0
                alive[res.made] = 3                             # (an old ghost that was touched again stays one)
                return rec.killed, rec.made, rec.killed_ghosts
            c["stat_sweep_bails"] += 1
            if undecided and res.max_cand < 9:
                c["stat_sweep_why"] |= SW_BAIL_M
        elif redo:
            c["stat_sweep_bails"] += 1                          # invalidate.h:92-93: a redone call counts as a bail for M
            c["stat_sweep_why"] |= SW_BAIL_M
        if not heap_ok:
            return None                                         # the heap needs the exact mask: nothing has been changed
        rec.killed = flood(path, sc, cn)
        return rec.killed, none, none

    valid = nf
    if soma:
        # trace.hip:211-218: one call around the root, ghosts not allowed, before the valid voxels are counted
        killed, _, _ = invalidate(-1, [root], soma_invalidation_scale, soma_invalidation_const, False, False, True, "soma")
        valid -= killed.size
        check_sound(-1, [root], soma_invalidation_scale, soma_invalidation_const)
    implicit = not before and not soma
    if implicit:
        before = [far]
    nb, na = len(before), len(after)
    max_paths = valid if max_paths is None else int(max_paths)
    paths, psave = [], []                                       # psave[k][i]: the weight vertex i of path k had before it became a rail
    result = lambda: SimpleNamespace(paths=paths[:c["n_paths"]], calls=calls, rollbacks=rollbacks, counters=c, soma=soma, root=root,
                                     ghosts_at_end=int(np.count_nonzero(alive == 3)), max_n_many=max_n_many[0], voxels=nf)
    if nb + na >= max_paths:
        return result()
    if fix_branching:
        pdrf[K.loc_of(root, shape)] = 0.0
    npaths = 0
    nghost = 0
    journal = []
    gs = None                                                   # GhostState: where a roll-back returns to
    redo = False
    open_ghost_calls = 0                                        # calls that made a ghost since the state a roll-back returns to
    while npaths < max_paths:
        reason = None
        if nghost > 0 and (valid == 0 or paranoid or no_journal):      # trace.hip:240
            reason = "paranoid" if paranoid else "no journal" if no_journal else "valid == 0"
        path = None
        if reason is None and not redo:
            if not (valid > 0 or nb > 0 or na > 0):
                break
            if nb > 0:
                nb -= 1
                target = before[nb]
            elif valid == 0:
                na -= 1
                target = after[na]
            else:
                first = order[np.flatnonzero(alive[order])[0]]         # ghosts count as alive here: their byte is not zero
                if nghost > 0 and alive[first] == 3:
                    reason = "ghost target"                            # trace.hip:268
                target = K.pt_of(int(first), shape)
            if reason is None:
                target = tuple(int(v) for v in target)
                if fix_branching:
                    path = K.railroad(PDRF, target)
                else:
                    path = K.path_to_source(PDRF, field_dist, root, target)
                if soma:                                               # trace.py:246-251
                    d = np.linalg.norm(np.asarray(anisotropy, dtype=np.float32) * (np.asarray(path) - np.asarray(root)), axis=1)
                    path = np.concatenate((path[:1, :], path[d > soma_radius, :]))
                if len(path) == 0:
                    break
                del paths[npaths:], psave[npaths:]
                paths.append(np.asarray(path))
        elif reason is None:
            path = paths[npaths]                                       # the path whose invalidation is redone (plens[npaths])
        if reason is None and valid > 0:
            if nghost == 0:
                gs = SimpleNamespace(paths=npaths, valid=valid, nb=nb, na=na)
                journal = []
            go_ghost = ghosts_on and not redo
            got = invalidate(npaths, path, scale, const, go_ghost, redo, nghost == 0, "redo" if redo else "sweep")
            if got is None:
                reason = "sweep abandoned"                             # trace.hip:359-360
            else:
                killed, made, gkilled = got
                valid -= killed.size + made.size
                if go_ghost:
                    nghost += made.size - gkilled.size
                    # the call's log: everything it killed (ghosts among them), then the ghosts it made (sweep.h:1030)
                    journal = journal + killed.tolist() + gkilled.tolist() + made.tolist() if nghost else []
                    if made.size:
                        c["stat_ghost_calls"] += 1
                        open_ghost_calls += 1
                    if nghost == 0:
                        open_ghost_calls = 0
                assert nghost == int(np.count_nonzero(alive == 3))
                check_sound(npaths, path, scale, const)
        if reason is not None:
            # trace.hip:388-404: the journal's voxels are alive again, the rails of the later paths get their weights back; the
            # path of the call that is redone stays a rail
            assert nghost > 0 and gs is not None and gs.paths < npaths
            alive[np.asarray(journal, dtype=np.int64)] = 1
            nrails = rail_paths = 0
            if fix_branching:
                for k in range(gs.paths + 1, npaths):
                    back = [(v, w) for v, w in zip(_locs(paths[k], shape).tolist(), psave[k]) if w != 0.0]
                    for v, w in back:
                        pdrf[v] = w
                    nrails += len(back)
                    rail_paths += 1 if back else 0
            rollbacks.append(SimpleNamespace(reason=reason, at=npaths, to=gs.paths, journal=len(journal), rails=nrails,
                                             rail_paths=rail_paths, ghost_calls_since=open_ghost_calls))
            open_ghost_calls = 0
            npaths, valid, nb, na = gs.paths, gs.valid, gs.nb, gs.na
            nghost, journal = 0, []
            c["stat_rollbacks"] += 1
            redo = True
            if soundness:
                # the oracle's own mask goes back as well: it is flooded again, path by path, from the redone call on
                exact[...] = labels
                exact_done[0] = -2
                if soma:
                    K.roll_invalidation_ball_inside_component(exact, DBF, soma_invalidation_scale, soma_invalidation_const, anisotropy,
                                                              [root], voxel_connectivity_graph=vcg)
                for k in range(npaths):
                    K.roll_invalidation_ball_inside_component(exact, DBF, scale, const, anisotropy, paths[k], voxel_connectivity_graph=vcg)
                exact_done[0] = npaths - 1
            continue
        redo = False
        if fix_branching:
            v = _locs(path, shape)
            del psave[npaths:]
            psave.append(pdrf[v].tolist())                             # (vertex by vertex as the kernel's loop: a vertex twice
            pdrf[v] = 0.0                                              #  in one path keeps its weight in both slots)
        npaths += 1
        c["n_paths"] = npaths
    c["n_paths"] = npaths
    c["n_vertices"] = int(sum(len(p) for p in paths[:npaths]))
    return result()
