"""The control cost of include/sfw_hip.h (sfw_sequences_control_cost) restated in numpy.

Pure numpy, no GPU.  For sample t of a perturbed stage with normals z[k][c][t] (perturb.normals, or the device's own from
sfw_sequences_normals), nominal plan nominal[k][c] and standard deviations sigma[c]:
  acc = +0.0
  for k = 0 .. K-1:  for c = 0, 1, 2 with sigma[c] > 0:
      q = nominal[k][c] / sigma[c];  acc = acc + q * z[k][c][t]      (division, product and sum: one rounding each)
  c_t = acc;  bias_t = gamma * c_t
which is u_nom^T Sigma^-1 eps_t for the unclamped eps = sigma * z.  The loop over (k, c) runs in Python in exactly this
order and every step is one elementwise numpy operation over the samples, so that with the device's normals handed in the
device's vector is reproduced bit for bit.
"""
import numpy as np


def control_cost(nominal, sigma, z, gamma):
    """gamma * c_t for every sample: nominal (K, 3), sigma (3,), z (K, 3, n) -> (n,) float64."""
    nominal = np.asarray(nominal, dtype=np.float64)
    if nominal.ndim != 2 or nominal.shape[1] != 3:
        raise ValueError("nominal must be a (K, 3) array")
    K = nominal.shape[0]
    sigma = np.asarray(sigma, dtype=np.float64).reshape(3)
    z = np.asarray(z, dtype=np.float64)
    if z.ndim != 3 or z.shape[:2] != (K, 3):
        raise ValueError("z must be a (K, 3, n) array")
    gamma = float(gamma)
    if not (np.all(np.isfinite(nominal)) and np.all(np.isfinite(sigma)) and np.isfinite(gamma)):
        raise ValueError("non-finite nominal, sigma or gamma")
    if np.any(sigma < 0.0):
        raise ValueError("sigma >= 0")
    acc = np.zeros(z.shape[2], dtype=np.float64)
    for k in range(K):
        for c in range(3):
            if not sigma[c] > 0.0:
                continue
            q = nominal[k, c] / sigma[c]       # one rounding
            acc = acc + q * z[k, c]            # product, then sum: one rounding each
    return np.float64(gamma) * acc
