"""Device-resident bf16 classifier running on the hand-written MFMA kernels.

Weights mirror models/classifier.HashedTextClassifier (the fp32 CPU oracle):
  h = gelu(feats @ w1 + b1); p = sigmoid(h @ w2 + b2)
W1 is stored transposed [H, D] (the GEMM consumes B^T), W2 transposed [C, H]
for the skinny gemv head. Numerics: bf16 inputs/weights, fp32 accumulate.
"""

from __future__ import annotations

import torch

from ..models.classifier import HashedTextClassifier
from ..ops import hip


# Largest row count the 64x64-tile GEMM takes: the largest measured M at
# which it still beats gemm_bt's 256x256 tiles (table: docs/kernels.md,
# "gemm_skinny"; 8192 rows and up were not measured and stay on gemm_bt).
SKINNY_MAX_M = 4096


class GpuClassifier:
    def __init__(self, model: HashedTextClassifier, device: str = "cuda"):
        self.dim = model.dim
        self.hidden = model.hidden
        self.classes = model.classes
        assert self.dim % 64 == 0 and self.hidden % 128 == 0, "MFMA tile constraints"
        with torch.no_grad():
            self.w1t = model.w1.t().contiguous().to(device=device, dtype=torch.bfloat16)  # [H, D]
            self.b1 = model.b1.to(device=device, dtype=torch.float32).contiguous()
            self.w2t = model.w2.t().contiguous().to(device=device, dtype=torch.bfloat16)  # [C, H]
            self.b2 = model.b2.to(device=device, dtype=torch.float32).contiguous()

    def _gemm(self, m: int):
        """The hidden-layer GEMM for m rows: the 64x64-tile kernel up to
        SKINNY_MAX_M rows (FORGE_GEMM_SKINNY=0 turns it off), else gemm_bt's
        v2 / v1. All three give the same bits."""
        if m <= SKINNY_MAX_M and hip.gemm_skinny_enabled() and hip.gemm_skinny_fits(m, self.hidden, self.dim):
            return hip.gemm_bt_skinny
        return hip.gemm_bt

    def forward(self, feats_bf16: torch.Tensor) -> torch.Tensor:
        """feats [Bpad, D] bf16 (Bpad%128==0) → probabilities fp32 [Bpad, C]."""
        gemm = self._gemm(feats_bf16.shape[0])
        h = gemm(feats_bf16, self.w1t, self.b1, act=hip.ACT_GELU, out_bf16=True)
        return hip.gemv_head(h, self.w2t, self.b2, act=hip.ACT_SIGMOID)

    def forward_into(self, feats_bf16: torch.Tensor, h_buf: torch.Tensor,
                     scores_buf: torch.Tensor) -> None:
        """Capture-safe forward: writes into preallocated buffers."""
        gemm = self._gemm(feats_bf16.shape[0])
        gemm(feats_bf16, self.w1t, self.b1, act=hip.ACT_GELU, out_bf16=True, out=h_buf)
        hip.gemv_head(h_buf, self.w2t, self.b2, act=hip.ACT_SIGMOID, out=scores_buf)
