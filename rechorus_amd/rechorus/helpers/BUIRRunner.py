"""BUIRRunner on the HIP engine (counterpart of the reference's helpers/BUIRRunner.py).

BUIR keeps two target tables that no gradient reaches: after EVERY optimizer step they move towards the online tables,
target = target * m + online * (1 - m).  That is the one thing this runner adds to BaseRunner: the per-batch order is zero_grad,
forward, loss, backward, optimizer.step(), model._update_target(), and the epoch loss is the mean of the batch means.  The loop
itself is BaseRunner.fit -- device-assembled batches without a sampler launch (BUIR.Dataset draws no negatives), dense HipOptimizer
updates (the reference's semantics), and with --graph 1 the step replayed from a hipGraph -- which calls `_after_step` behind each
step; the target update is ONE launch (rc_buir_ema) issued there, outside the captured graph.
"""
from helpers.BaseRunner import BaseRunner


class BUIRRunner(BaseRunner):
    def _use_rowwise(self, model) -> bool:
        # a row-wise step would have to move the target rows lazily as well: a different optimiser, not offered
        if self.engine == 'rowwise':
            raise ValueError('BUIRRunner has no row-wise step (--engine rowwise): the target tables follow dense updates')
        return False

    def _after_step(self, model):
        model._update_target()
