"""The reference's `dataloaders` package, as far as this build carries it: `utils.post_processing` (and
`utils.post_processing_volume`, the same function handed a volume) beside the label-map helpers.  Loading and augmentation
live in ustrun/datasets.py and ustrun/synthetic.py."""
