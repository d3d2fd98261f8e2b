"""PGGAN, ResNet architecture -- drop-in for PGGAN/model_resnet.py of the reference, the network its train.py builds by default
(`--model resnet`, PGGAN/train.py:49,62-67).

`PGGAN(args)` keeps the reference interface: `args.block_count` (number of up / down blocks: resolution 4 * 2**block_count),
`args.trans` (fade-in of the newest block), `args.inputs_norm`; `get_generator(z_var, alpha, training, reuse)` and
`get_discriminator(x_var, alpha, labels, update_collection, reuse)` under the scopes `g_net` / `d_net` (:14-70).  The networks
themselves are common.resnet_block.Generator_PGGAN / Discriminator_PGGAN.  Images are bf16 NHWC [N, H, W, 3].
"""
from ..common import resnet_block as _blocks
from ..store import get_default_store


class PGGAN(object):
    def __init__(self, args):
        self.bc = args.block_count  # Count of up/down block.
        self.trans = args.trans  # If trans.
        self.inputs_norm = args.inputs_norm

    def get_generator(self, z_var, alpha, training=True, reuse=False):
        """(:24-38) z_var [N, z_dim] bf16 -> images [N, 4 * 2**bc, 4 * 2**bc, 3]"""
        store = get_default_store()
        with store.variable_scope('g_net', reuse=reuse):
            z_var_ = z_var.reshape(z_var.shape[0], -1)
            return _blocks.Generator_PGGAN(z_var_, self.bc, self.trans, alpha, self.inputs_norm, training=training)

    def get_discriminator(self, x_var, alpha, labels=None, update_collection=None, reuse=False):
        """(:40-70) x_var [N, H, W, 3] -> logits [N]; `labels` is handed on as the critic's (unused) c_var, as in the reference"""
        store = get_default_store()
        with store.variable_scope('d_net', reuse=reuse):
            c_code = labels
            return _blocks.Discriminator_PGGAN(x_var, c_code, self.bc, self.trans, alpha, self.inputs_norm,
                                               update_collection=update_collection, reuse=reuse)
