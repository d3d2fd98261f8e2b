"""The Inception score's statistics restated in NumPy float64, for the tests of gan_lib_tensorflow_amd/common/inception/
inception_score.py and csrc/inception_score.hip: a stable softmax of the first 1000 logits, then the formula of `preds2score`
(exp of the mean over a split's rows of KL(p(y|x) || p(y)), splits sliced as i*n//splits), with log p taken as the
log-softmax l - lse and terms of probability 0 counted as 0 -- the same number as `p * log p` wherever that is finite."""
import numpy as np

N_CLASSES = 1000


def log_softmax(logits):
    """float64 [n, 1000] log-probabilities of the first 1000 columns"""
    l = np.asarray(logits)[:, :N_CLASSES].astype(np.float64)
    l = l - l.max(axis=1, keepdims=True)
    return l - np.log(np.exp(l).sum(axis=1, keepdims=True))


def bounds(n, splits):
    return [i * n // splits for i in range(splits + 1)]


def state(logits, splits):
    """float64 [splits, 1001]: per split the class-probability sums, then sum_x sum_y p log p"""
    logp = log_softmax(logits)
    p = np.exp(logp)
    b = bounds(len(logp), splits)
    out = np.zeros((splits, N_CLASSES + 1))
    for i in range(splits):
        part, lpart = p[b[i]:b[i + 1]], logp[b[i]:b[i + 1]]
        out[i, :N_CLASSES] = part.sum(axis=0)
        out[i, N_CLASSES] = (part * lpart).sum()
    return out


def scores(logits, splits):
    """float64 [splits]: exp(mean_x sum_y p (log p - log m)), m the split's mean probability"""
    logp = log_softmax(logits)
    p = np.exp(logp)
    b = bounds(len(logp), splits)
    out = []
    for i in range(splits):
        part, lpart = p[b[i]:b[i + 1]], logp[b[i]:b[i + 1]]
        marginal = part.mean(axis=0, keepdims=True)
        with np.errstate(divide='ignore', invalid='ignore'):
            terms = np.where(part > 0, part * (lpart - np.log(marginal)), 0.0)
        out.append(np.exp(terms.sum(axis=1).mean()))
    return np.asarray(out)


def score(logits, splits):
    s = scores(logits, splits)
    return np.mean(s), np.std(s)
