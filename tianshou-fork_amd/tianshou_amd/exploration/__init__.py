"""Action noise processes (tianshou/exploration/random.py)."""
from tianshou_amd.exploration.random import BaseNoise, GaussianNoise, OUNoise

__all__ = ["BaseNoise", "GaussianNoise", "OUNoise"]
