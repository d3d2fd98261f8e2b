"""Float64 restatement of the FID statistics and distance for the tests (imports nothing from the product):
np.cov statistics, the Frechet distance in its published scipy.linalg.sqrtm form (`.real`, no eps branch), and the
thresholded eigen form that the product states (eigenvalues below D * 2^-52 * lambda_max count as zero)."""
import numpy as np


def statistics(features):
    x = np.asarray(features, dtype=np.float64)
    return x.mean(axis=0), np.cov(x, rowvar=False)


def frechet_sqrtm(mu1, sigma1, mu2, sigma2):
    from scipy import linalg
    covmean = linalg.sqrtm(sigma1.dot(sigma2))
    if isinstance(covmean, tuple):          # older SciPy returns (sqrtm, error estimate) under disp=False only; be safe
        covmean = covmean[0]
    covmean = covmean.real
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def _clip(w, d):
    w = w.copy()
    w[w < d * 2.0 ** -52 * w.max()] = 0.0
    w[w < 0.0] = 0.0
    return w


def frechet_eigen(mu1, sigma1, mu2, sigma2):
    d = mu1.shape[0]
    lam, vec = np.linalg.eigh(sigma1)
    half = vec @ np.diag(np.sqrt(_clip(lam, d))) @ vec.T
    inner = half @ sigma2 @ half
    lam2 = np.linalg.eigvalsh(0.5 * (inner + inner.T))
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.sqrt(_clip(lam2, d)).sum())


def bf16_round(x):
    import torch
    return torch.tensor(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def feature_sets(d, n, seed=0, count=2):
    """`count` sets of relu(N(0,1) A + 0.3), each with its own random D x D mixing matrix A, rounded to bfloat16; float64 [n, d]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        a = rng.normal(size=(d, d)) / np.sqrt(d)
        out.append(bf16_round(np.maximum(rng.normal(size=(n, d)) @ a + 0.3, 0.0)))
    return out
