"""Label embedding -- drop-in for common/ops/embedding.py of the reference."""
import numpy as np

from ... import functional as Fn
from ...store import get_default_store
from . import sn as _sn


def embedding_variable(vocab_size=1000, embedding_dim=300, word2vec_file=None):
    """The variable half of embed_y (embedding.py:28-40): `Embedding.Label/embedding_map` [vocab, dim], U(+-0.08) or the
    word2vec table (then not trainable)."""
    store = get_default_store()
    with store.variable_scope("Embedding.Label"):
        if word2vec_file is None:
            return store.get_variable('embedding_map', [vocab_size, embedding_dim],
                                      lambda rng: rng.uniform(low=-0.08, high=0.08,
                                                              size=(vocab_size, embedding_dim)).astype('float32'),
                                      trainable=True)
        return store.get_variable('embedding_map', None, np.asarray(word2vec_file, 'float32'), trainable=False)


def normalized_embedding_variable(vocab_size=1000, embedding_dim=300, word2vec_file=None, update_collection=None):
    """The table of embedding_variable divided by its spectral norm, E / sigma(E): the reference's `spectral_normed_weight`
    (sn.py:15-69) on the [vocab, dim] matrix, u [1, dim] stored as `Embedding.Label/embedding_map/spectral_norm/u`, one power
    iteration, `update_collection` as everywhere else (None: u is overwritten on every execution; NO_OPS: read, never written).
    Inside `sn.precomputed` the table is one of the network's batched weights (sn.sn_pairs knows the name)."""
    table = embedding_variable(vocab_size, embedding_dim, word2vec_file)
    store = get_default_store()
    dim = table.shape[-1]
    with store.variable_scope("Embedding.Label"), store.variable_scope("embedding_map"), store.variable_scope("spectral_norm"):
        u = store.get_variable('u', [1, dim], lambda rng: _sn._trunc_normal(rng, (1, dim)), trainable=False)
    return _sn.spectral_normed_weight(table, u=u, update_collection=update_collection)


def embed_y(inputs, vocab_size=1000, embedding_dim=300, word2vec_file=None,
            spectral_normed=False, update_collection=None, reuse=False):
    """inputs: int32 [batch]; returns bf16 [batch, embedding_dim] (embedding.py:12-51).  spectral_normed: the rows come from the
    normalised table (the switch the reference's signature carries and its body ignores)."""
    if spectral_normed:
        return Fn.embedding(normalized_embedding_variable(vocab_size, embedding_dim, word2vec_file, update_collection), inputs)
    return Fn.embedding(embedding_variable(vocab_size, embedding_dim, word2vec_file), inputs)
