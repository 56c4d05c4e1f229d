"""The reference's `dataloaders` package, as far as this build carries it: `utils.post_processing`.  Loading and augmentation
live in ustrun/datasets.py and ustrun/synthetic.py."""
