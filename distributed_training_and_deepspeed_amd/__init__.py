"""MI355X-native distributed training (DDP, GPipe / stage-per-process pipelines, ZeRO 0-3) with
hand-written gfx950 kernels; see README.md."""
