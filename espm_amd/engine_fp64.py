"""fp64 mode of the device engine: ``MUEngine(..., precision="fp64")``.

The log_surrogate multiplicative updates (espm/estimators/updates.py:6-156) in double precision, with the reference's simplex
bisection and its global stop (dicotomy.py:4-55, :111-173), on the kernels of csrc/mu_fp64.hip.  The reference computes in
fp64 unless X is float32 (base.py:243-247); with a small ``tol`` its stop rules compare numbers at fp32 rounding level, so only
this mode follows its trajectories.

Data layout in HBM (torch tensors):
  x      (n, p) u8|bf16|f32|f64   X channel-major, in the narrowest store that holds every value exactly; the kernels
                                  read (double) x * xscale
  sp     the sparse store          instead of x for a sparse image of integer counts (x_store "sparse", espm_amd/sparse64.py):
                                  its non-zero elements in two orders, on the kernels of csrc/mu_fp64_sparse.hip
  h[2]   (k, p) f64               ping-pong H
  w[2]   (M, k) f64               ping-pong W (M = m, or n when G is the identity)
  gw     (n, k) f64               G W, its column sums, a flag "an entry is below log_shift"
  hist   (max_iter + 3, 8) f64    per state: sum(Y - X log Y), sum mu log(H + eps), sum H (H L), rel_W, rel_H

Scope: 1..8 components, one GPU, G identity / dictionary / refreshed by a physics model (set_G), mu scalar or per
component, the grid or identity Laplacian, simplex_H or simplex_W (with a physics model's rows), fixed_H, fixed_W.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, sparse64
from .conf import dicotomy_tol as DICOTOMY_TOL, maxit_dichotomy as MAXIT
from .engine import MUEngine, _ptr, _stream, require_gpu

_STORES = {"u8": _lib.F64_X_U8, "bf16": _lib.F64_X_BF16, "f32": _lib.F64_X_F32, "f64": _lib.F64_X_F64}
_KL, _REG, _LAP, _REL_W, _REL_H = range(5)


def _exact_store(Xd):
    """The narrowest store that holds every value of the fp64 device array Xd exactly: u8, bf16, f32 or f64."""
    if bool(((Xd == torch.round(Xd)) & (Xd >= 0) & (Xd <= 255)).all()):
        return "u8"
    if bool((Xd.to(torch.bfloat16).to(torch.float64) == Xd).all()):
        return "bf16"
    if bool((Xd.to(torch.float32).to(torch.float64) == Xd).all()):
        return "f32"
    return "f64"


class MUEngineF64(MUEngine):
    """One SmoothNMF problem resident on one GPU, every array and every operation in fp64.  Same methods as MUEngine for the
    scope above; the arguments outside it raise NotImplementedError."""

    def __init__(self, X, n_components, *, layout="cm", G=None, shape_2d=None, lambda_L=0.0, mu=0, epsilon_reg=1.0,
                 simplex_H=False, simplex_W=True, log_shift=1e-14, dicotomy_tol=DICOTOMY_TOL, tol=1e-4, sigmaL=8.0,
                 fixed_H=None, fixed_W=None, simplex_rows=None, xscale=1.0, x_store="auto", max_iter=200, device=None,
                 group=None, fix_zero_lines=True, precision="fp64", bregman=False, h_rule=0, frobenius=False, filled_channels=None,
                 filled_pixels=None, **ignored):
        if group is not None:
            raise NotImplementedError("fp64 mode runs on one GPU: no sharded engine")
        if bregman or h_rule or frobenius:
            raise NotImplementedError("fp64 mode: only the log_surrogate multiplicative updates")
        k = int(n_components)
        if not 1 <= k <= _lib.F64_MAX_K:
            raise NotImplementedError(f"fp64 mode: n_components = {k} (the fp64 kernels are built for 1..{_lib.F64_MAX_K} components)")
        self.device = dev = require_gpu(device)
        self.group, self.world, self.rank, self.sharded, self.frobenius = None, 1, 0, False, False
        self.precision = "fp64"
        self.k = k
        self.V = _lib.variant(k)
        self.lib, self._check = self.V.lib, self.V.check
        f64 = dict(dtype=torch.float64, device=dev)

        # ---- X: (n, p) channel-major on the device, in a store that holds it exactly ------------------------------------
        Xt = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X))
        if Xt.dim() != 2:
            raise ValueError("X must be 2-D")
        if layout not in ("cm", "pm"):
            raise ValueError("layout must be 'cm' or 'pm'")
        self.out_dtype = np.float64
        self.xscale = float(xscale)
        self.sp, self.x, self.x_type = None, None, None
        self.x_store_note = None   # (why 'auto' kept an image dense, if it did)
        if x_store in ("auto", "sparse"):
            # one pass over X in row chunks in its own dtype (a host array goes up chunk by chunk: no fp64 copy of the image)
            stats = sparse64.scan(Xt, layout, x_store, filled_channels=filled_channels, filled_pixels=filled_pixels, device=dev)
            use, note = sparse64.choose(stats, x_store)
            if use:
                self.sp = sparse64.build(stats, fix_zero_lines)
                self.n, self.p, self.p_total = stats["n"], stats["p"], stats["p"]
                self.x_store = "sparse"
                self.c_kl, self.sum_x = sparse64.constants(self.sp, self.xscale, log_shift)
            else:
                self.x_store_note = note
            del stats
        if self.sp is None:
            self.x_store = self._dense_store(Xt, layout, x_store, fix_zero_lines, log_shift)
        del Xt

        # ---- G, parameters ------------------------------------------------------------------------------------------------
        self.m = 0 if G is None else int(np.asarray(G).shape[1])
        self.M = self.n if G is None else self.m
        self.g = self.colsum_g = None
        if G is not None:
            Gh = np.asarray(G, dtype=np.float64)
            if Gh.shape[0] != self.n:
                raise ValueError(f"G must have {self.n} rows, got {Gh.shape}")
            self.g = torch.from_numpy(np.ascontiguousarray(Gh)).to(dev)
            self.colsum_g = torch.from_numpy(Gh.sum(axis=0)).to(dev)
        if shape_2d is not None:
            nx, ny = (int(shape_2d[0]), int(shape_2d[1]))
            if nx * ny != self.p:
                raise ValueError(f"shape_2d {shape_2d} does not match {self.p} pixels")
            self.nx, self.ny = nx, ny
        else:
            self.nx, self.ny = 0, 0
        self.lambda_L, self.sigma = float(lambda_L), float(sigmaL)
        self.eps_reg, self.log_shift = float(epsilon_reg), float(log_shift)
        self.dicotomy_tol, self.rel_tol = float(dicotomy_tol), float(tol)
        self.simplex_H, self.simplex_W = bool(simplex_H), bool(simplex_W)
        self.mu = torch.from_numpy(np.broadcast_to(np.asarray(mu, dtype=np.float64), (k,)).copy()).to(dev)
        self.fixed_h = self._dev(fixed_H, (k, self.p), "fixed_H") if fixed_H is not None else None
        self.fixed_w = self._dev(fixed_W, (self.M, k), "fixed_W") if fixed_W is not None else None
        self.rows, self.nrows = None, self.M
        if simplex_rows is not None:
            mask = np.zeros(self.M, dtype=np.uint8)
            mask[np.asarray(simplex_rows)] = 1
            self.rows, self.nrows = torch.from_numpy(mask).to(dev), int(mask.sum())
        if self.simplex_W and log_shift > 0 and self.nrows * log_shift >= 1:
            raise ValueError("No solution exists!")
        if self.simplex_H and log_shift > 0 and k * log_shift >= 1:
            raise ValueError("No solution exists!")

        # ---- state and workspaces -----------------------------------------------------------------------------------------
        self.w = [torch.zeros((self.M, k), **f64) for _ in range(2)]
        self.h = [torch.ones((k, self.p), **f64) for _ in range(2)]
        self.gw = torch.zeros((self.n, k), **f64)
        self.colsum_gw = torch.zeros(k, **f64)
        self.gw_small = torch.zeros(1, dtype=torch.int32, device=dev)
        self.hstat = torch.zeros(2 * k, **f64)
        self.rh = torch.zeros((self.n, k), **f64)
        self.numden = torch.zeros((2, k, self.p), **f64) if self.simplex_H else None
        self.mask = torch.zeros(2, dtype=torch.int64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        need = max(int(self.lib.espm_f64_scratch_doubles(self.n, self.p, k, k * self.p)),
                   int(self.lib.espm_f64_scratch_doubles(self.n, self.p, k, self.M * k)),
                   int(self.lib.espm_f64_sparse_scratch_doubles(self.n, self.p, k)) if self.sp is not None else 0)
        self.scratch = torch.zeros(need, **f64)
        self.hist_len = int(max_iter) + 3
        self.hist = torch.zeros((self.hist_len, 8), **f64)
        self.cur, self.it = 0, 0
        self._h_ready = None   # (cur, it) of an H update eval_current left in h[1 - cur]

    def _dense_store(self, Xt, layout, x_store, fix_zero_lines, log_shift):
        """X (n, p) channel-major on the device in a dense store that holds it exactly; const_KL and sum_x of the effective X."""
        dev, f64 = self.device, dict(dtype=torch.float64, device=self.device)
        Xd = Xt.to(device=dev, dtype=torch.float64)
        if layout == "pm":
            Xd = Xd.t()
        elif layout != "cm":
            raise ValueError("layout must be 'cm' or 'pm'")
        Xd = Xd.contiguous()
        n, p = Xd.shape
        self.n, self.p, self.p_total = int(n), int(p), int(p)
        if bool((Xd < 0).any()):
            raise ValueError("Negative values in data")  # espm/estimators/base.py:528
        if fix_zero_lines:   # base.py:519-528
            zp, zc = Xd.sum(dim=0) == 0, Xd.sum(dim=1) == 0
            Xd[:, zp] = log_shift
            Xd[zc, :] = log_shift
        store = _exact_store(Xd) if x_store == "auto" else x_store
        if store not in _STORES:
            raise ValueError(f"fp64 mode: x_store must be 'auto', 'sparse', 'u8', 'bf16', 'f32' or 'f64', got {x_store!r}")
        if store != "f64" and _STORES[store] < _STORES[_exact_store(Xd)]:
            raise ValueError(f"fp64 mode: X does not fit the {store} store exactly")
        self.x_store, self.x_type = store, _STORES[store]
        self.x = {"u8": lambda t: t.to(torch.uint8), "bf16": lambda t: t.to(torch.bfloat16), "f32": lambda t: t.to(torch.float32),
                  "f64": lambda t: t}[store](Xd).contiguous()
        # const_KL (base.py:200-201) of the effective X, in row chunks
        total = torch.zeros((), **f64)
        step = max(1, (32 << 20) // max(1, self.p))
        for a in range(0, self.n, step):
            xs = Xd[a:a + step] * self.xscale
            total += (xs * torch.log(xs.clamp_min(log_shift))).sum() - xs.sum()
        self.c_kl = float(total)
        self.sum_x = float(Xd.sum()) if self.xscale == 1.0 else float((Xd * self.xscale).sum())
        del Xd
        return store

    # ---- helpers ----------------------------------------------------------------------------------------------------------------
    def _dev(self, a, shape, name):
        t = a.to(device=self.device, dtype=torch.float64) if isinstance(a, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(self.device)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
        return t.contiguous()

    def _build_gw(self, which):
        g = self.g if self.m else None
        self._check(self.lib.espm_f64_gw(_ptr(g), _ptr(self.w[which]), self.n, self.m, self.k, self.log_shift, _ptr(self.gw),
                                         _ptr(self.colsum_gw), _ptr(self.gw_small), _stream()))

    def _hstat(self, h):
        self._check(self.lib.espm_f64_hstat(_ptr(h), self.k, self.p, self.log_shift, _ptr(self.scratch), _ptr(self.hstat), _stream()))

    def _h_update(self, src, dst, slot, mode_update=True):
        """The pass over X for state (w[src] via gw, h[src]): loss pieces -> hist[slot]; with mode_update the new H in h[dst]."""
        if self.lambda_L != 0:
            self._hstat(self.h[src])
        mode = 0 if not mode_update else (2 if self.simplex_H else 1)
        num, den = (self.numden[0], self.numden[1]) if mode == 2 else (None, None)
        if self.sp is not None:
            sp = self.sp
            head = (self.lib.espm_f64_sparse_h_pass, (_ptr(sp["h_elem"]), _ptr(sp["h_off"]), _ptr(sp["ec"]), sp["n_ec"], _ptr(sp["ep_flag"])))
        else:
            head = (self.lib.espm_f64_h_pass, (_ptr(self.x), self.x_type))
        self._check(head[0](
            *head[1], self.n, self.p, self.xscale, _ptr(self.gw), _ptr(self.colsum_gw), _ptr(self.gw_small),
            _ptr(self.h[src]), self.k, _ptr(self.hstat), _ptr(self.mu), self.eps_reg, self.lambda_L, self.sigma, self.nx, self.ny,
            self.log_shift, mode, _ptr(self.fixed_h), _ptr(self.h[dst]) if mode == 1 else None, _ptr(num), _ptr(den),
            _ptr(self.scratch), _ptr(self.hist[slot]), _stream()))
        if mode == 2:
            self._check(self.lib.espm_f64_bisect(_ptr(num), _ptr(den), self.k, self.p, self.log_shift, self.dicotomy_tol, MAXIT,
                                                 _ptr(self.fixed_h), _ptr(self.h[dst]), _ptr(self.mask), _ptr(self.status), _stream()))

    def _w_update(self, w_src, h_src, w_dst):
        """W update from w[w_src] (its G W is current) with H = h[h_src] into w[w_dst]."""
        self._hstat(self.h[h_src])
        if self.sp is not None:
            sp = self.sp
            head = (self.lib.espm_f64_sparse_w_accum, (_ptr(sp["w_elem"]), _ptr(sp["w_off"]), _ptr(sp["ec_flag"]), _ptr(sp["ep"]), _ptr(sp["ep_off"])))
        else:
            head = (self.lib.espm_f64_w_accum, (_ptr(self.x), self.x_type))
        self._check(head[0](*head[1], self.n, self.p, self.xscale, _ptr(self.gw), _ptr(self.h[h_src]), self.k, self.log_shift,
                            _ptr(self.scratch), _ptr(self.rh), _stream()))
        g = self.g if self.m else None
        self._check(self.lib.espm_f64_w_finish(_ptr(self.rh), _ptr(g), _ptr(self.colsum_g), self.n, self.m, self.k, _ptr(self.w[w_src]),
                                               _ptr(self.hstat), int(self.simplex_W), _ptr(self.rows), self.nrows, self.log_shift,
                                               DICOTOMY_TOL, MAXIT, _ptr(self.fixed_w), _ptr(self.w[w_dst]), _ptr(self.status), _stream()))

    def _rel(self, new, old, out):
        self._check(self.lib.espm_f64_rel(_ptr(new), _ptr(old), new.numel(), self.rel_tol, _ptr(self.scratch), _ptr(out), _stream()))

    # ---- the MUEngine interface -------------------------------------------------------------------------------------------------
    def load_state(self, W, H):
        """Install (W, H) as the current state, in fp64 (no rounding on the way), and build G W."""
        Wt = self._dev(W, (self.M, self.k), "W")
        Ht = self._dev(H, (self.k, self.p), "H")
        self.cur, self.it, self._h_ready = 0, 0, None
        self.hist.zero_()
        self.status.zero_()
        self.w[0].copy_(Wt)
        self.h[0].copy_(Ht)
        self._build_gw(0)

    def set_G(self, G):
        """Replace G (a physics model refreshed it, espm/estimators/base.py:388-390) and rebuild G W."""
        if self.m == 0:
            raise ValueError("the engine was built with G = identity")
        Gh = np.ascontiguousarray(np.asarray(G, dtype=np.float64))
        if Gh.shape != (self.n, self.m):
            raise ValueError(f"G must stay {(self.n, self.m)}, got {Gh.shape}")
        self.g.copy_(torch.from_numpy(Gh))
        self.colsum_g.copy_(torch.from_numpy(Gh.sum(axis=0)))
        self._h_ready = None
        self._build_gw(self.cur)

    def eval_current(self, advance_h=True):
        """Loss pieces of the current state into history slot ``it``; with advance_h the H update in the other buffer and rel_H
        of the next state."""
        cur, slot = self.cur, self.it
        if advance_h:
            if slot + 1 >= self.hist_len:
                raise ValueError("history buffer exhausted: raise max_iter")
            self._h_update(cur, 1 - cur, slot)
            self._rel(self.h[1 - cur], self.h[cur], self.hist[slot + 1, _REL_H:_REL_H + 1])
            self._h_ready = (cur, slot)
        else:
            self._h_update(cur, 1 - cur, slot, mode_update=False)

    def finish_iteration(self):
        """W update with the H eval_current produced, rel_W, G W of the new W; flips the buffers."""
        cur, slot = self.cur, self.it
        if self._h_ready != (cur, slot):
            raise RuntimeError("finish_iteration needs the H update of eval_current(advance_h=True) first")
        self._w_update(cur, 1 - cur, 1 - cur)
        self._rel(self.w[1 - cur], self.w[cur], self.hist[slot + 1, _REL_W:_REL_W + 1])
        self._build_gw(1 - cur)
        self._h_ready = None
        self.cur, self.it = 1 - cur, slot + 1

    def iterate(self, n_iter, final_loss=True):
        """``n_iter`` iterations without host synchronisation (no stop criterion)."""
        if self.it + n_iter + 1 > self.hist_len:
            raise ValueError("history buffer exhausted: raise max_iter")
        for _ in range(int(n_iter)):
            self.eval_current(True)
            self.finish_iteration()
        if final_loss:
            self.eval_current(False)

    def step_h_only(self, l2=False):
        """The H update of the current state (multiplicative_step_h); returns it, the state is unchanged."""
        if l2:
            raise NotImplementedError("fp64 mode: no Frobenius branch")
        self._h_update(self.cur, 1 - self.cur, self.hist_len - 1)
        self._h_ready = None
        self._raise_status()
        return self.h[1 - self.cur].cpu().numpy()

    def step_w_only(self, l2=False):
        """The W update with the CURRENT H (multiplicative_step_w); returns it, the state is unchanged."""
        if l2:
            raise NotImplementedError("fp64 mode: no Frobenius branch")
        self._w_update(self.cur, self.cur, 1 - self.cur)
        self._h_ready = None
        self._raise_status()
        return self.w[1 - self.cur].cpu().numpy()

    def _raise_status(self):
        if int(self.status.item()):
            self.status.zero_()
            raise AssertionError("dichotomy_simplex preconditions violated")  # dicotomy.py:17-19, :141-144

    def get_W(self):
        return self.w[self.cur].cpu().numpy()

    def get_H(self):
        return self.h[self.cur].cpu().numpy()

    def bad_count(self):
        return 0.0

    def history(self, upto=None, average=True):
        """Loss pieces of states 0..upto (inclusive) assembled like SmoothNMF.loss (espm/estimators/smooth_nmf.py:457-475)."""
        upto = self.it if upto is None else upto
        h = self.hist[:upto + 1].cpu().numpy()
        self._raise_status()
        numel = float(self.n) * float(self.p) if average else 1.0
        kl = (h[:, _KL] + self.c_kl) / numel
        reg = h[:, _REG] / numel
        lap = 0.5 * self.lambda_L * h[:, _LAP] / numel
        return dict(loss=kl + reg + lap, kl=kl, reg=reg, lap=lap, rel_W=h[:, _REL_W], rel_H=h[:, _REL_H], bad=np.zeros(len(h)))

    # ---- what the fp64 engine does not have -------------------------------------------------------------------------------------
    def _unsupported(self, *a, **k):
        raise NotImplementedError("fp64 mode: not available (single-GPU log_surrogate updates only)")

    autotune_plan = settle_exchange = use_collective_exchange = linesearch_step = pg_linesearch_h = pg_linesearch_w = _unsupported
    iterate_timed = timed_iterations = advance_h_only = iterate_h = _unsupported
