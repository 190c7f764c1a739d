"""Manifold learning on the device: exact t-SNE (tsne.py, csrc/tsne.hip)."""
from .tsne import TSNE

__all__ = ["TSNE"]
