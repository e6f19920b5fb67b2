#!/usr/bin/env python
"""Bits of the 16-lane kernels (vjp_kernel, pw_kernel, gains_kernel) from one library against another's.

    MPCB_LIB=.../lib_a.so python tools/bits_calls.py record a.npz
    python tools/bits_calls.py record b.npz
    python tools/bits_calls.py compare a.npz b.npz

``record`` runs one call programme on the library that MPCB_LIB names (default: the tree's) and
keeps every output array, status and return code.  ``compare`` exits 0 only if the two files hold the
same keys and every array is identical bit for bit (NaN payloads included).  No reference and no
oracle: what is compared is one build of the library with another.

The programme: mpcb_solve_vjp, _w, _vjp_pw (with and without the weight gradients),
mpcb_solve_iterate_pw, _pm, mpcb_solve_gains and _pm (no mask, the ``U`` route, the ``fixed`` route), on
handles with and without an input box, in fp64 and fp32, with and without wind, at
  B in {1, 7, 70}: three padding groups; a partial last wave; with one workspace slot
                   (MPCB_VJP_SLOTS = MPCB_PW_SLOTS = MPCB_GAINS_SLOTS = 1, set by the caller) the stride
                   loop reuses the slot and the LDS;
  N in {1, 8, 17, 64}: only lane 0 owns a stage; fewer stages than lanes; lane 0 owns two; the top
                   bit of the stage masks.
Every call holds one NaN instance (B // 2, in xbar); B = 1 is run once more without it.  As a guard
that the two processes saw the same inputs, mpcb_solve_iterate (the tuned solve path, other
kernels) and mpcb_qp_stats are recorded too, and so are the inputs.  A refused call is recorded by its
return code.  Run each recording in a fresh process.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FILL = 777.0   # outputs start from this, so what a call does not write compares equal as well


def record(path):
    import numpy as np
    import torch

    from mpc_blaster_amd import BatchedMPC, MPCConfig
    out = {}
    ncalls = 0

    def keep(tag, rc, **arrays):
        nonlocal ncalls
        ncalls += 1
        out[f'{tag}/rc'] = np.int64(rc)
        for k, v in arrays.items():
            out[f'{tag}/{k}'] = v.detach().cpu().numpy()

    def programme(m, tag, B, N, box, wind, nan):
        dt, dev, lib = m.dtype, m._tdev, m.lib
        P, null, st = m._ptr, m._ptr(None), m._stream()
        seed = 1000 + 7 * B + N
        inp = m.gen_inputs(B, seed=seed, ref='sine', wind=wind)
        x0, xr, ur, wd = inp['x0'], inp['xref'], inp['uref'], inp['wind']
        xr_sb, wd_p, wd_sb = (N + 1) * 12, (P(wd) if wind else null), (3 if wind else 0)
        m.solve(x0, xr, ur, wind=wd)   # the iterate: one rollout-mode step
        xbar, ubar = m.get_state_trajectory().clone(), m.get_input_trajectory().clone()
        if nan:
            xbar[B // 2, 0, 3] = float('nan')
        gen = torch.Generator(device='cpu').manual_seed(seed)

        def rnd(*shape):
            return torch.randn(shape, dtype=torch.float64, generator=gen).to(dtype=dt, device=dev)

        def congruent(W):
            W = torch.as_tensor(np.asarray(W, dtype=np.float64), dtype=dt, device=dev)
            e = torch.exp(0.35 * rnd(B, W.shape[0]))
            return (W[None] * e[:, :, None] * e[:, None, :]).contiguous()
        gX, gU = rnd(B, N + 1, 12), rnd(B, N, 4)
        Qw, Rw, QNw = congruent(m.cfg.Q), congruent(m.cfg.R), congruent(m.cfg.QN)
        model = m.pack_model(B, mass=m.cfg.mass * (1 + 0.2 * torch.rand(B, generator=gen).to(dt).to(dev)),
                             t_blast=5.0 * torch.rand(B, generator=gen).to(dt).to(dev), J=congruent(m.cfg.J))
        fixed = (torch.rand((B, N, 4), generator=gen) < 0.4).to(torch.uint8).to(dev)

        def new(*shape):
            return torch.full(shape, FILL, dtype=dt, device=dev)

        def status():
            return torch.full((B,), 777, dtype=torch.int32, device=dev)
        keep(f'{tag}/inputs', 0, x0=x0, xref=xr, uref=ur, xbar=xbar, ubar=ubar, model=model)

        # the guard: the tuned solve path and its statistics
        u0, X, U, s = new(B, 4), new(B, N + 1, 12), new(B, N, 4), status()
        rc = lib.mpcb_solve_iterate(m._h, B, P(x0), 12, P(xbar), P(ubar), P(xr), xr_sb, P(ur), 0, wd_p, wd_sb,
                                    P(u0), P(X), P(U), P(s), st)
        qs = torch.full((B, 2), 777, dtype=torch.int32, device=dev)
        rc2 = lib.mpcb_qp_stats(m._h, B, P(qs), st)
        keep(f'{tag}/solve_iterate', rc, u0=u0, X=X, U=U, status=s)
        keep(f'{tag}/qp_stats', rc2, stats=qs)
        Ub = P(U) if box else null   # the products' and the gains' active set

        # the products
        def vjp_outs(wg):
            o = dict(gx0=new(B, 12), gxref=new(B, N + 1, 12), guref=new(B, N, 4), status=status())
            if wg:
                o.update(gQ=new(B, 12, 12), gR=new(B, 4, 4), gQN=new(B, 12, 12))
            return o
        o = vjp_outs(False)
        rc = lib.mpcb_solve_vjp(m._h, B, P(xbar), P(ubar), Ub, wd_p, wd_sb, P(gX), P(gU), P(o['gx0']), P(o['gxref']),
                                P(o['guref']), P(o['status']), st)
        keep(f'{tag}/vjp', rc, **o)
        o = vjp_outs(False)   # gx0 alone: no forward pass
        rc = lib.mpcb_solve_vjp(m._h, B, P(xbar), P(ubar), Ub, wd_p, wd_sb, P(gX), null, P(o['gx0']), null, null,
                                P(o['status']), st)
        keep(f'{tag}/vjp_gx0', rc, **o)
        o = vjp_outs(True)
        rc = lib.mpcb_solve_vjp_w(m._h, B, P(xbar), P(ubar), P(X), P(U), P(xr), xr_sb, P(ur), 0, wd_p, wd_sb, P(gX),
                                  P(gU), P(o['gx0']), P(o['gxref']), P(o['guref']), P(o['gQ']), P(o['gR']), P(o['gQN']),
                                  P(o['status']), st)
        keep(f'{tag}/vjp_w', rc, **o)
        for wg in (False, True):
            o = vjp_outs(wg)
            g3 = (P(o['gQ']), P(o['gR']), P(o['gQN'])) if wg else (null, null, null)
            rc = lib.mpcb_solve_vjp_pw(m._h, B, P(xbar), P(ubar), P(X), P(U), P(xr), xr_sb, P(ur), 0, wd_p, wd_sb,
                                       P(Qw), 144, P(Rw), 16, P(QNw), 144, P(gX), P(gU), P(o['gx0']), P(o['gxref']),
                                       P(o['guref']), *g3, P(o['status']), st)
            keep(f'{tag}/vjp_pw{int(wg)}', rc, **o)

        # the step with per-instance weights and vehicles (fp32 with the box: refused, by its code)
        for name, md in (('pw', None), ('pm', model)):
            o = dict(u0=new(B, 4), X=new(B, N + 1, 12), U=new(B, N, 4), status=status())
            head = [m._h, B, P(x0), 12, P(xbar), P(ubar), P(xr), xr_sb, P(ur), 0, wd_p, wd_sb, P(Qw), 144, P(Rw), 16,
                    P(QNw), 144]
            tail = [P(o['u0']), P(o['X']), P(o['U']), P(o['status']), st]
            rc = (lib.mpcb_solve_iterate_pw(*head, *tail) if md is None else
                  lib.mpcb_solve_iterate_pm(*head, P(md), 14, *tail))
            keep(f'{tag}/{name}', rc, **o)

        # the gains: the handle's route (U on a box handle), the `fixed` bytes, K alone
        for route, Ua, fa in (('U', Ub, null), ('fixed', null, P(fixed))):
            for name, md in (('gains', None), ('gains_pm', model)):
                o = dict(K=new(B, N, 4, 12), P0=new(B, 12, 12), status=status())
                head = [m._h, B, P(xbar), P(ubar), Ua, fa, wd_p, wd_sb]
                tail = [P(o['K']), P(o['P0']) if route == 'U' else null, P(o['status']), st]
                rc = (lib.mpcb_solve_gains(*head, *tail) if md is None else
                      lib.mpcb_solve_gains_pm(*head, P(md), 14, *tail))
                keep(f'{tag}/{name}_{route}', rc, **o)
        torch.cuda.synchronize()

    for dtype in ('f64', 'f32'):
        for N in (1, 8, 17, 64):
            for box in (False, True):
                # a box tight enough around the hover thrust that components clamp
                probe = BatchedMPC(MPCConfig(N=N, dtype=dtype), max_batch=1)
                uh = probe.gen_inputs(1, seed=1)['uref'][0, 0].double().cpu().numpy()
                del probe
                m = BatchedMPC(MPCConfig(N=N, dtype=dtype, lbu=uh - 0.5 if box else None,
                                         ubu=uh + 0.5 if box else None), max_batch=70)
                for B in (1, 7, 70):
                    for wind in (False, True):
                        for nan in ((True, False) if B == 1 else (True,)):
                            programme(m, f'{dtype}/N{N}/box{int(box)}/B{B}/wind{int(wind)}/nan{int(nan)}',
                                      B, N, box, wind, nan)
                del m
    np.savez_compressed(path, **out)
    print(f'{path}: {ncalls} calls, {len(out)} arrays, library {os.environ.get("MPCB_LIB", "(the tree)")}')


def compare(pa, pb):
    import numpy as np
    a, b = np.load(pa), np.load(pb)
    ka, kb = set(a.files), set(b.files)
    bad = sorted(ka ^ kb)
    groups = {}   # (dtype, call, array) -> [arrays that differ, largest relative difference]
    for k in sorted(ka & kb):
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            bad.append(k)
            p = k.split('/')
            g = groups.setdefault((p[0], p[-2], p[-1]), [0, 0.0])
            g[0] += 1
            if x.shape == y.shape and x.dtype.kind == 'f':
                with np.errstate(all='ignore'):
                    d = np.abs(x.astype(np.float64) - y.astype(np.float64)) / np.maximum(np.abs(x.astype(np.float64)), 1e-300)
                d = np.where(np.isnan(x) & np.isnan(y), 0.0, np.where(np.isnan(d), np.inf, d))
                g[1] = max(g[1], float(d.max()))
    written = sum(1 for k in ka & kb if not k.endswith('/rc') and '/inputs/' not in k)
    accepted = sum(1 for k in ka if k.endswith('/rc') and int(a[k]) == 0)
    print(f'{len(ka)} / {len(kb)} arrays ({written} outputs; {accepted} calls accepted), {len(bad)} differ')
    for g, (n, d) in sorted(groups.items()):
        print(f'  differs: {"/".join(g)}: {n} arrays, largest relative difference {d:.3g}')
    for k in bad[:8]:
        print('  e.g.', k)
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == 'record':
        record(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
