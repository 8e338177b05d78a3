"""Kernel- and mean-function parameter objects (host side).

Mirrors the parameter containers of the reference (`src/kernels.jl:59-76,109-131,174-187`,
`src/means.jl:7-18`). They hold hyper-parameters only: all kernel-matrix arithmetic runs in
the HIP library (`csrc/`), reached through the C ABI in `include/dsmgp_hip.h`.

Parametrisation (reference `src/kernels.jl:68-73`, `src/gaussianprocess.jl:39`):
  lengthscale = exp(logl), signal variance = exp(2*logs), noise variance = exp(2*logNoise).
Hyper-vector layout per kernel id: [logl..., logs, logNoise] (`src/gaussianprocess.jl:153-161`).
"""
import numpy as np

# numeric kinds shared with include/dsmgp_hip.h
KIND_ISO_SE = 0
KIND_ARD_SE = 1
KIND_ISO_LINEAR = 2
KIND_ARD_LINEAR = 3
KIND_ARD_SE_PRODUCT = 4
KIND_ISO_MATERN32 = 5
KIND_ISO_MATERN52 = 6
KIND_ARD_MATERN32 = 7
KIND_ARD_MATERN52 = 8
KIND_ISO_RQ = 9
KIND_ARD_RQ = 10


class KernelFunction:
    kind = -1

    def loghyp(self):
        """[logl..., logs] on the log scale (variance slot is a dummy 0.0 for IsoLinear)."""
        raise NotImplementedError

    def set_loghyp(self, v):
        raise NotImplementedError

    def nparams(self):
        return len(self.loghyp())

    def copy(self):
        raise NotImplementedError


class IsoSE(KernelFunction):
    """k(a,b) = exp(2 logs) * exp(-0.5 |a-b|^2 / exp(logl)^2)  (`src/kernels.jl:59-83`)."""
    kind = KIND_ISO_SE

    def __init__(self, logl, logs):
        self.logl = float(logl)
        self.logs = float(logs)
        self.dl = 0.0
        self.ds = 0.0

    def loghyp(self):
        return np.array([self.logl, self.logs])

    def set_loghyp(self, v):
        self.logl, self.logs = float(v[0]), float(v[1])

    def copy(self):
        return IsoSE(self.logl, self.logs)

    def __repr__(self):
        return f"IsoSE({self.logl}, {self.logs})"


class ArdSE(KernelFunction):
    """ADDITIVE ARD kernel exp(2 logs) * sum_d exp(-0.5 (a_d-b_d)^2 / exp(logl_d)^2)
    (`src/kernels.jl:31-49,109-144`: `umap!` accumulates per dimension)."""
    kind = KIND_ARD_SE

    def __init__(self, logl, logs):
        self.logl = np.array(logl, dtype=np.float64).reshape(-1)
        self.logs = float(logs)
        self.dl = np.zeros_like(self.logl)
        self.ds = 0.0

    def loghyp(self):
        return np.concatenate([self.logl, [self.logs]])

    def set_loghyp(self, v):
        self.logl = np.array(v[:-1], dtype=np.float64)
        self.logs = float(v[-1])

    def copy(self):
        return ArdSE(self.logl.copy(), self.logs)

    def __repr__(self):
        return f"ArdSE({self.logl.tolist()}, {self.logs})"


class IsoLinear(KernelFunction):
    """k(a,b) = a.b / exp(logl)^2; the variance slot is a dummy (`src/kernels.jl:174-194`)."""
    kind = KIND_ISO_LINEAR

    def __init__(self, logl):
        self.logl = float(logl)
        self.dl = 0.0

    def loghyp(self):
        return np.array([self.logl, 0.0])

    def set_loghyp(self, v):
        self.logl = float(v[0])  # setvariance! is a no-op (`src/kernels.jl:183`)

    def copy(self):
        return IsoLinear(self.logl)

    def __repr__(self):
        return f"IsoLinear({self.logl})"


class ArdLinear(KernelFunction):
    """k(a,b) = sum_d a_d b_d / exp(logl_d)^2 over the D input dimensions; the variance slot is a dummy
    (`src/kernels.jl:209-230` through the generic ArdKernel loop `:39-49`).  The reference's own ArdLinear cannot be fitted
    (`:232,247`); this is the kernel its generic code states.  Length-scale gradients are the true derivatives of the
    log-marginal (include/dsmgp_hip.h, dsmgp_gradients)."""
    kind = KIND_ARD_LINEAR

    def __init__(self, logl):
        self.logl = np.array(logl, dtype=np.float64).reshape(-1)
        self.dl = np.zeros_like(self.logl)

    def loghyp(self):
        return np.concatenate([self.logl, [0.0]])

    def set_loghyp(self, v):
        self.logl = np.array(v[:-1], dtype=np.float64)  # setvariance! is a no-op (`src/kernels.jl:218`)

    def copy(self):
        return ArdLinear(self.logl.copy())

    def __repr__(self):
        return f"ArdLinear({self.logl.tolist()})"


class ArdSEProduct(KernelFunction):
    """Product-form ARD squared exponential exp(2 logs) * exp(-0.5 sum_d (a_d-b_d)^2 / exp(logl_d)^2) over the D input
    dimensions (GPML's covSEard).  Not a kernel of the reference, whose ArdSE is additive.  Same hyper-vector
    layout as ArdSE; all gradients are the true derivatives of the log-marginal (include/dsmgp_hip.h, dsmgp_gradients)."""
    kind = KIND_ARD_SE_PRODUCT

    def __init__(self, logl, logs):
        self.logl = np.array(logl, dtype=np.float64).reshape(-1)
        self.logs = float(logs)
        self.dl = np.zeros_like(self.logl)
        self.ds = 0.0

    def loghyp(self):
        return np.concatenate([self.logl, [self.logs]])

    def set_loghyp(self, v):
        self.logl = np.array(v[:-1], dtype=np.float64)
        self.logs = float(v[-1])

    def copy(self):
        return ArdSEProduct(self.logl.copy(), self.logs)

    def __repr__(self):
        return f"ArdSEProduct({self.logl.tolist()}, {self.logs})"


class _IsoMatern(KernelFunction):
    """Matern kernel with one length-scale: exp(2 logs) (1 + s [+ s^2/3]) exp(-s), s = sqrt(2 nu) |a-b| / exp(logl)
    (GPML's covMaterniso).  Not a kernel of the reference.  Hyper-vector [logl, logs] as IsoSE; the gradients are the true
    derivatives of the log-marginal (no SURVEY F7 factor sigma; include/dsmgp_hip.h, dsmgp_gradients)."""

    def __init__(self, logl, logs):
        self.logl = float(logl)
        self.logs = float(logs)
        self.dl = 0.0
        self.ds = 0.0

    def loghyp(self):
        return np.array([self.logl, self.logs])

    def set_loghyp(self, v):
        self.logl, self.logs = float(v[0]), float(v[1])

    def copy(self):
        return type(self)(self.logl, self.logs)

    def __repr__(self):
        return f"{type(self).__name__}({self.logl}, {self.logs})"


class _ArdMatern(KernelFunction):
    """Matern kernel with one length-scale per input dimension: r^2 = sum_d (a_d-b_d)^2 / exp(logl_d)^2 in the formula of
    the iso kind (GPML's covMaternard, the distance form).  Not a kernel of the reference.  Hyper-vector [logl_1..logl_D,
    logs] as ArdSEProduct; all gradients are the true derivatives of the log-marginal."""

    def __init__(self, logl, logs):
        self.logl = np.array(logl, dtype=np.float64).reshape(-1)
        self.logs = float(logs)
        self.dl = np.zeros_like(self.logl)
        self.ds = 0.0

    def loghyp(self):
        return np.concatenate([self.logl, [self.logs]])

    def set_loghyp(self, v):
        self.logl = np.array(v[:-1], dtype=np.float64)
        self.logs = float(v[-1])

    def copy(self):
        return type(self)(self.logl.copy(), self.logs)

    def __repr__(self):
        return f"{type(self).__name__}({self.logl.tolist()}, {self.logs})"


class IsoMatern32(_IsoMatern):
    """Matern nu = 3/2: exp(2 logs) (1 + s) exp(-s), s = sqrt(3) |a-b| / exp(logl)."""
    kind = KIND_ISO_MATERN32


class IsoMatern52(_IsoMatern):
    """Matern nu = 5/2: exp(2 logs) (1 + s + s^2/3) exp(-s), s = sqrt(5) |a-b| / exp(logl)."""
    kind = KIND_ISO_MATERN52


class ArdMatern32(_ArdMatern):
    """Matern nu = 3/2 with per-dimension length-scales: s = sqrt(3 sum_d (a_d-b_d)^2 / exp(logl_d)^2)."""
    kind = KIND_ARD_MATERN32


class ArdMatern52(_ArdMatern):
    """Matern nu = 5/2 with per-dimension length-scales: s = sqrt(5 sum_d (a_d-b_d)^2 / exp(logl_d)^2)."""
    kind = KIND_ARD_MATERN52


class IsoRQ(KernelFunction):
    """Rational quadratic kernel with one length-scale (GPML's covRQiso): exp(2 logs) (1 + w)^(-alpha), w = |a-b|^2 /
    (2 alpha exp(logl)^2), alpha = exp(loga) -- a scale mixture of squared exponentials whose shape alpha is trained with the
    rest.  Not a kernel of the reference.  Hyper-vector [logl, loga, logs]; the gradients dl, da, ds are the true derivatives
    (include/dsmgp_hip.h, dsmgp_gradients)."""
    kind = KIND_ISO_RQ

    def __init__(self, logl, loga, logs):
        self.logl = float(logl)
        self.loga = float(loga)
        self.logs = float(logs)
        self.dl = 0.0
        self.da = 0.0
        self.ds = 0.0

    def loghyp(self):
        return np.array([self.logl, self.loga, self.logs])

    def set_loghyp(self, v):
        self.logl, self.loga, self.logs = float(v[0]), float(v[1]), float(v[2])

    def copy(self):
        return IsoRQ(self.logl, self.loga, self.logs)

    def __repr__(self):
        return f"IsoRQ({self.logl}, {self.loga}, {self.logs})"


class ArdRQ(KernelFunction):
    """Rational quadratic kernel with one length-scale per input dimension (GPML's covRQard): w = sum_d (a_d-b_d)^2 /
    (2 alpha exp(logl_d)^2) in the formula of IsoRQ.  Not a kernel of the reference.  Hyper-vector [logl_1..logl_D, loga, logs];
    all gradients are the true derivatives."""
    kind = KIND_ARD_RQ

    def __init__(self, logl, loga, logs):
        self.logl = np.array(logl, dtype=np.float64).reshape(-1)
        self.loga = float(loga)
        self.logs = float(logs)
        self.dl = np.zeros_like(self.logl)
        self.da = 0.0
        self.ds = 0.0

    def loghyp(self):
        return np.concatenate([self.logl, [self.loga, self.logs]])

    def set_loghyp(self, v):
        self.logl = np.array(v[:-2], dtype=np.float64)
        self.loga = float(v[-2])
        self.logs = float(v[-1])

    def copy(self):
        return ArdRQ(self.logl.copy(), self.loga, self.logs)

    def __repr__(self):
        return f"ArdRQ({self.logl.tolist()}, {self.loga}, {self.logs})"


class ConstMean:
    """Constant mean function (`src/means.jl:7-18`)."""

    default = False      # True: the builder's own mean(y[obs]) of the leaf (no meanFun given); add_data lets it follow the grown list

    def __init__(self, m, default=False):
        self.m = float(m)
        if default:
            self.default = True

    def __repr__(self):
        return f"ConstMean({self.m})"
