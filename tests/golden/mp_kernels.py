"""The kernel kinds of include/dsmgp_hip.h entry by entry in mpmath, once, for the generators of the 50-digit fixtures, with the
helpers they share.  The same table as tests/dense_kernels.py in other arithmetic: `h` is the hyper-vector without the noise
as mp numbers, (il2, al, s2) = unpack(kind, h, D) is taken once per case, and every derivative is the TRUE one."""
import io
import zipfile

import mpmath as mp
import numpy as np

ARD = (1, 3, 4, 7, 8, 10)
LINEAR = (2, 3)
RQ = (9, 10)


def unpack(kind, h, D):
    """(1 / l_d^2 per dimension, alpha or None, sigma^2 (1 for the linear kinds))."""
    nl = D if kind in ARD else 1
    il2 = [1 / mp.e ** (2 * h[d if kind in ARD else 0]) for d in range(D)]
    al = mp.e ** h[nl] if kind in RQ else None
    return il2, al, (mp.mpf(1) if kind in LINEAR else mp.e ** (2 * h[nl + (1 if kind in RQ else 0)]))


def _radial(kind, r2, al, s2):
    """(k, c) with dk / d(r^2) = -c / 2, for the kinds that are functions of r^2 = sum_d (a_d - b_d)^2 / l_d^2 alone."""
    if kind in (0, 4):
        k = s2 * mp.e ** (-r2 / 2)
        return k, k
    if kind in RQ:
        w = r2 / (2 * al)
        k = s2 * mp.e ** (-al * mp.log(1 + w))
        return k, k / (1 + w)
    nu2 = 3 if kind in (5, 7) else 5
    s = mp.sqrt(nu2 * r2)
    k = s2 * mp.e ** (-s) * (1 + s + (s * s / 3 if nu2 == 5 else 0))
    return k, s2 * mp.e ** (-s) * (1 if nu2 == 3 else (1 + s) / 3) * nu2


def value(kind, a, b, il2, al, s2):
    if kind == 1:
        return s2 * mp.fsum(mp.e ** (-((p - q) ** 2) * il / 2) for p, q, il in zip(a, b, il2))
    if kind in LINEAR:
        return mp.fsum(p * q * il for p, q, il in zip(a, b, il2))
    return _radial(kind, mp.fsum((p - q) ** 2 * il for p, q, il in zip(a, b, il2)), al, s2)[0]


def d_hyper(kind, a, b, il2, al, s2):
    """(k, [dk / dtheta per slot of h]); the dummy variance slot of the linear kinds is zero."""
    if kind in LINEAR:
        prod = [p * r * il for p, r, il in zip(a, b, il2)]
        k = mp.fsum(prod)
        return k, ([-2 * v for v in prod] if kind in ARD else [-2 * k]) + [mp.mpf(0)]
    q = [(p - r) ** 2 * il for p, r, il in zip(a, b, il2)]
    if kind == 1:
        e = [s2 * mp.e ** (-qd / 2) for qd in q]
        k = mp.fsum(e)
        return k, [ed * qd for ed, qd in zip(e, q)] + [2 * k]
    r2 = mp.fsum(q)
    k, c = _radial(kind, r2, al, s2)
    per = [c * qd for qd in q]
    dk = per if kind in ARD else [mp.fsum(per)]
    if kind in RQ:
        w = r2 / (2 * al)
        dk = dk + [k * al * (w / (1 + w) - mp.log(1 + w))]
    return k, dk + [2 * k]


def mll_convention(kind, h, dk):
    """The slots as dsmgp_gradients contracts them (ArdSE option on): the reference's factor sigma on both IsoSE slots and on
    the ArdSE variance slot."""
    if kind == 0:
        return [mp.e ** h[1] * v for v in dk]
    if kind == 1:
        return dk[:-1] + [mp.e ** h[-1] * dk[-1]]
    return dk


def d_input(kind, xt, xi, il2, al, s2):
    """dk(x_t, x_i) / dx_{t,d} for every d, for the kinds that are functions of r^2 alone."""
    c = _radial(kind, mp.fsum((p - q) ** 2 * il for p, q, il in zip(xt, xi, il2)), al, s2)[1]
    return [-c * (p - q) * il for p, q, il in zip(xt, xi, il2)]


def spread_logl(D, lo=0.7, hi=1.4):
    """log l_d spread over [lo, hi] times 0.35 sqrt(D), the length-scales of the per-family fixtures."""
    return np.log(0.35 * np.sqrt(D) * np.linspace(lo, hi, D)) if D > 1 else np.log([0.35])


def iso_logl(D):
    return np.log([0.35 * np.sqrt(D)])


def savez_reproducible(path, arrays, compresslevel=None):
    """np.savez_compressed with sorted keys, fixed member timestamps and modes: a rerun writes the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=compresslevel) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue(), compresslevel=compresslevel)
