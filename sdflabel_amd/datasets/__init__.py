"""Datasets of the reference that this package ports: datasets.crops (the CSS network's training crops)."""
