"""
Linked channels (include/pv_koala_batch.h, LINKED CHANNELS; DESIGN.md section 2, eighth extension) restated from the oracle's stages:
linked(planar x) for B = G C streams whose groups of C share one mask.  Shared by tests/test_channel_link.py (CPU) and
tests/test_gpu_channel_link.py; not a test module.

Per frame: spectrum X and raw mask m of every stream as tests/frame_report_recipe.ReportRecipe.stages gives them; koala_amd.channels.link_masks
for the rule; frame_report_recipe.applied_mask for the limit, per stream; oracle.synthesis with a tail kept per stream.  Report rows through
frame_report_recipe.report_rows with the linked mask -- e_out is of the linked m' -- and mask_sum from the raw one.
A handle with channels takes interleave(x) and gives interleave(linked(x)).
"""
import numpy as np

from frame_report_recipe import F32, ReportRecipe, applied_mask, report_rows, row_sum
from koala_amd.channels import link_masks
from oracle import oracle


class LinkRecipe:
    def __init__(self, model, B, C, precision='fp32', link=True):
        if B % C:
            raise ValueError('num_streams %d is not a multiple of channels %d' % (B, C))
        link_masks(np.zeros((C, 1), F32), C)  # (C = 1, 3, 5, 6, 7: refused, as the handle refuses them)
        self.r = ReportRecipe(model, B, precision)
        self.B, self.C, self.link = B, C, link
        self.tail = np.zeros((B, 256), F32)

    def reset(self, rows):
        rows = np.asarray(rows, bool)
        self.r.reset(rows)
        self.tail[rows] = 0

    def process(self, x, gains=None, reset=None):
        """x int16 planar [B, T * 256] -> (enhanced int16 [B, T * 256], report float32 [B, T, 4]); reset [B, T]: a stream is fresh right before
        that frame (it may differ within a group)"""
        x = np.ascontiguousarray(x, np.int16)
        T = x.shape[1] // 256
        g = np.zeros(self.B, F32) if gains is None else np.broadcast_to(np.asarray(gains, F32), (self.B,))
        out = np.empty_like(x)
        rep = np.empty((self.B, T, 4), F32)
        for t in range(T):
            if reset is not None:
                self.reset(np.asarray(reset)[:, t] != 0)
            spec, m = self.r.stages(x[:, t * 256:(t + 1) * 256])  # [B, 1, 257, 2], [B, 1, 257]
            ml = link_masks(m, self.C) if self.link else m
            for b in range(self.B):
                out[b, t * 256:(t + 1) * 256] = oracle.synthesis(spec[b, 0], applied_mask(ml[b, 0], g[b]), self.tail[b])
                rep[b, t] = report_rows(spec[b, 0], ml[b, 0], g[b])
                rep[b, t, 2] = row_sum(m[b, 0])
        return out, rep
