"""The linear baseline: a ridge regression from time-lagged brain sensors to speech features (the backward mTRF).

Every decoding result is compared with a linear decoder on the same segments, scored by the same retrieval; the field's is
`mne.decoding.TimeDelayingRidge` / `ReceptiveField`.  `LaggedRidge` is that estimator with `edge_correction=False` (the
autocorrelation method) and lags l = 0 ... L - 1, the brain following the speech:

    yhat_b(t) = ybar + sum_l W_l^T x_b(t + l)

Every segment is zero outside [0, T) in x and in y - ybar, and the squared error is summed over every t at which a term is
non-zero.  The normal equations are then exactly block-Toeplitz:

    A_d[i][j] = sum_b sum_u x_b[u + d, i] x_b[u, j]        G[(l, c), (l', c')] = A_{l - l'}[c][c'] for l >= l', transposed otherwise
    R_l[c][f] = sum_b sum_t x_b[t + l, c] y_b[t, f]        s_l[c] = sum_b sum_{u >= l} x_b[u, c]
    (G + alpha I) W = R - s ybar^T                         ybar = sum y / (B T)

in sklearn's Ridge convention (alpha on the un-normalised Gram matrix, x not centred).

Where it runs.  `partial_fit` copies X and Y into lag-layout buffers (rows of channels, C padded to 64, H = L - 1 zero rows behind
every segment: a torch strided copy, plumbing) and runs `sda_lagged_cov_f32` (csrc/lagged_cov.hip, exact-fp32 MFMA) twice — the
A_d and the R_l; their slabs are summed in float64 and added to float64 accumulators on the device, as are s_l and sum y (small,
torch, float64).  Nothing is read back.  `solve` assembles G in float64 on the device by index gathers over the valid channels
and factors it once per alpha (torch.linalg.cholesky_ex + cholesky_solve; on the host in float64 if this torch build has no
device solver: `solver_` says which ran).  `predict` is the existing window GEMM (`sda_window_gemm_f32`) on the lag-layout
buffer: a C -> F convolution of width L is a fixed (L Cp, F) matrix applied to windows of L rows, one row apart; every requested
alpha sits side by side in its columns.

Not built: mne's edge correction, negative lags, a Toeplitz-aware solver, 16-bit operands for the products, data-parallel
fitting.  Parity with mne's own arrays is unpinned (mne is not a dependency of the tests); the estimator is pinned against
sklearn.linear_model.Ridge on the explicit design matrix (tests/test_ridge_cpu.py).
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import lib as L
from . import ops


def _need_segments(who: str, t, channels: int, what: str):
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[1] != channels:
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{who}: {what} must be (B, {channels}, T), got {got}")
    if not t.is_cuda:
        raise L.SdaError(f"{who}: {what} must live on the MI355X device (there is no CPU path)")
    if t.dtype not in ops.COMPUTE_DTYPES:
        raise L.SdaError(f"{who}: {what} of dtype {t.dtype}; segments are float32, bfloat16 or float16")


class LaggedRidge:
    """ridge = LaggedRidge(C, F, n_lags); ridge.partial_fit(X, Y) per batch; ridge.solve(alphas); ridge.predict(X);
    ridge.score(X, bank, labels).  After solve(): coef_ (n_alphas, L, C, F) fp32, intercept_ (F,) fp32, alphas_ (tuple)."""

    def __init__(self, C: int, F: int, n_lags: int = 60, device="cuda"):
        if int(C) < 1 or int(F) < 1 or int(n_lags) < 1:
            raise ValueError(f"LaggedRidge: C, F and n_lags must be positive, got C={C}, F={F}, n_lags={n_lags}")
        self.C, self.F, self.n_lags = int(C), int(F), int(n_lags)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SdaError("LaggedRidge runs on the MI355X device (there is no CPU path)")
        L.load()
        self.H = self.n_lags - 1                        # zero rows behind every segment in the lag layout
        self.Cp, self.Fp = L.pad_channels(self.C), L.pad_channels(self.F)
        f64 = dict(dtype=torch.float64, device=self.device)
        self.A = torch.zeros((self.n_lags, self.C, self.C), **f64)
        self.R = torch.zeros((self.n_lags, self.C, self.F), **f64)
        self.s = torch.zeros((self.n_lags, self.C), **f64)
        self.sum_y = torch.zeros((self.F,), **f64)
        self.n = 0                                      # B T over every batch (known on the host: no read-back)
        self._buffers = {}                              # "x" / "y" -> lag-layout buffer, pads zero, reused while the shape repeats
        self.coef_ = self.intercept_ = self.alphas_ = self.solver_ = self.best_alpha_ = None

    # ------------------------------------------------------------------------------------------------------ lag layout
    def _lag_rows(self, which: str, t: torch.Tensor, Cp: int) -> torch.Tensor:
        """(B, c, T) of any supported dtype and strides -> this shape's (B (T + H), Cp) fp32 buffer: segment b in rows
        b (T + H) ... + T - 1, channels-last.  Only valid rows and channels are ever written, so the pads stay zero."""
        B, c, T = t.shape
        buf = self._buffers.get(which)
        if buf is None or buf.shape[0] != B * (T + self.H):
            buf = self._buffers[which] = torch.zeros((B * (T + self.H), Cp), dtype=torch.float32, device=self.device)
        buf.view(B, T + self.H, Cp)[:, :T, :c].copy_(t.detach().transpose(1, 2))
        return buf

    # ------------------------------------------------------------------------------------------------------------- fit
    @torch.no_grad()
    def partial_fit(self, X: torch.Tensor, Y: torch.Tensor) -> "LaggedRidge":
        """Add the segments X (B, C, T) and Y (B, F, T) to the normal equations."""
        _need_segments("LaggedRidge.partial_fit", X, self.C, "X")
        _need_segments("LaggedRidge.partial_fit", Y, self.F, "Y")
        if X.shape[0] != Y.shape[0] or X.shape[2] != Y.shape[2] or X.shape[0] < 1 or X.shape[2] < 1:
            raise ValueError(f"LaggedRidge.partial_fit: X {tuple(X.shape)} and Y {tuple(Y.shape)} must share B >= 1 and T >= 1")
        B, _, T = X.shape
        Lg, C, F = self.n_lags, self.C, self.F
        with torch.cuda.device(self.device):
            xb = self._lag_rows("x", X, self.Cp)
            yb = self._lag_rows("y", Y, self.Fp)
            self.A += ops.lagged_cov(xb, xb, Lg, self.H).sum(dim=0, dtype=torch.float64)[:, :C, :C]
            self.R += ops.lagged_cov(xb, yb, Lg, self.H).sum(dim=0, dtype=torch.float64)[:, :C, :F]
            # s_l = sum over u >= l: the total minus the first l time steps (lags >= T see nothing)
            xt = xb.view(B, T + self.H, self.Cp)[:, :T, :C].sum(dim=0, dtype=torch.float64)           # (T, C)
            head = torch.cat([torch.zeros_like(xt[:1]), xt.cumsum(dim=0)], dim=0)                       # head[l] = sum_{u < l}
            lags = torch.arange(Lg, device=self.device).clamp_(max=T)
            self.s += head[T].unsqueeze(0) - head[lags]
            self.sum_y += yb.view(B, T + self.H, self.Fp)[:, :T, :F].sum(dim=(0, 1), dtype=torch.float64)
        self.n += B * T
        return self

    # ----------------------------------------------------------------------------------------------------------- solve
    def gram(self) -> torch.Tensor:
        """G (L C, L C) float64 on the device, assembled from the A_d by index gathers."""
        Lg, C = self.n_lags, self.C
        l = torch.arange(Lg, device=self.device)
        d = l[:, None] - l[None, :]                                        # (L, L'): l - l'
        blocks = self.A[d.abs()]                                           # (L, L', C, C') = A_|d|[c][c']
        blocks = torch.where((d >= 0)[:, :, None, None], blocks, blocks.transpose(-1, -2))
        return blocks.permute(0, 2, 1, 3).reshape(Lg * C, Lg * C)

    def rhs(self) -> torch.Tensor:
        """R - s ybar^T as (L C, F) float64 on the device."""
        if self.n < 1:
            raise L.SdaError("LaggedRidge: nothing has been fitted yet (call partial_fit first)")
        ybar = self.sum_y / self.n
        return (self.R - self.s[:, :, None] * ybar[None, None, :]).reshape(self.n_lags * self.C, self.F)

    @torch.no_grad()
    def solve(self, alphas: Sequence[float] = (1.0,)) -> "LaggedRidge":
        """(G + alpha I) W = R - s ybar^T for every alpha: coef_, intercept_, alphas_."""
        alphas = tuple(float(a) for a in alphas)
        if not alphas or any(not a >= 0 for a in alphas):
            raise ValueError(f"LaggedRidge.solve: alphas must be one or more numbers >= 0, got {alphas}")
        rhs, G = self.rhs(), self.gram()
        try:
            torch.linalg.cholesky_ex(torch.eye(2, dtype=torch.float64, device=self.device))
            self.solver_ = "device"
        except RuntimeError:                    # this torch build has no device solver: the same solve on the host, float64
            rhs, G = rhs.cpu(), G.cpu()
            self.solver_ = "host"
        coef = []
        for a in alphas:
            M = G.clone()
            M.diagonal().add_(a)
            chol, info = torch.linalg.cholesky_ex(M)
            del M
            if int(info) != 0:
                raise L.SdaError(f"LaggedRidge.solve: G + alpha I is not positive definite at alpha = {a:g} "
                                 f"(Cholesky stopped at minor {int(info)}); use a larger alpha")
            W = torch.cholesky_solve(rhs, chol)
            coef.append(W.reshape(self.n_lags, self.C, self.F).to(device=self.device, dtype=torch.float32))
        self.coef_ = torch.stack(coef)
        self.intercept_ = (self.sum_y / self.n).float()
        self.alphas_ = alphas
        self.best_alpha_ = None
        return self

    # --------------------------------------------------------------------------------------------------------- predict
    def window_matrix(self, alpha: Optional[int] = None) -> torch.Tensor:
        """The window GEMM's matrix (L Cp, n F) fp32: row l Cp + c, column a F + f = coef_[a, l, c, f]; pad channels zero rows."""
        if self.coef_ is None:
            raise L.SdaError("LaggedRidge: solve() has not run")
        coef = self.coef_ if alpha is None else self.coef_[int(alpha)][None]
        n = coef.shape[0]
        Bm = torch.zeros((self.n_lags, self.Cp, n, self.F), dtype=torch.float32, device=self.device)
        Bm[:, :self.C] = coef.permute(1, 2, 0, 3)
        return Bm.view(self.n_lags * self.Cp, n * self.F)

    @torch.no_grad()
    def predict(self, X: torch.Tensor, alpha: Optional[int] = None) -> torch.Tensor:
        """yhat (B, F, T) fp32 for alphas_[alpha], or (n_alphas, B, F, T) for all of them (alpha=None)."""
        from .signal_prep import window_gemm
        _need_segments("LaggedRidge.predict", X, self.C, "X")
        Bm = self.window_matrix(alpha)
        B, _, T = X.shape
        n = Bm.shape[1] // self.F
        with torch.cuda.device(self.device):
            xb = self._lag_rows("x", X, self.Cp)
            out = window_gemm(xb.view(B, (T + self.H) * self.Cp), Bm, T, self.Cp)             # (B, T n F)
            Z = (out.view(B, T, n, self.F) + self.intercept_).permute(2, 0, 3, 1).contiguous()
        return Z if alpha is None else Z[0]

    @torch.no_grad()
    def score(self, X: torch.Tensor, bank, labels, k: int = 10):
        """Decode the predictions of every alpha against `bank` (retrieval.retrieve with `labels`): the list of Retrievals, one
        per alpha.  topk_ / top1_ hold their accuracies, best_alpha_ the index of the best top-k (top-1, then the smaller alpha,
        decide a tie)."""
        from .retrieval import retrieve
        Z = self.predict(X)
        results = [retrieve(Z[i], bank, k=k, labels=labels) for i in range(Z.shape[0])]
        self.topk_ = [r.accuracy(k) for r in results]
        self.top1_ = [r.accuracy(1) for r in results]
        self.best_alpha_ = max(range(len(results)), key=lambda i: (self.topk_[i], self.top1_[i], -i))
        return results
