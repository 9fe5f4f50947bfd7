"""Counterpart of the reference's `utils` package: `eval_metrics` (the ORBIT benchmark's evaluators on the native per-video
metrics kernel). `utils.optim` of the reference lives in `orbit_dataset_amd.optim`."""
