"""BaseNoise, GaussianNoise and OUNoise (tianshou/exploration/random.py:7-85) on the host.

The draws come from NumPy's global stream with the reference's calls, shapes and order, so a
seeded run consumes the stream as the reference does; DDPGPolicy.exploration_noise uploads the
f64 draws and adds them on the device (tsrl_act_noise)."""
from abc import ABC, abstractmethod
from typing import Optional, Sequence, Union

import numpy as np


class BaseNoise(ABC):
    def __init__(self) -> None:
        super().__init__()

    def reset(self) -> None:
        """Back to the initial state."""

    @abstractmethod
    def __call__(self, size: Sequence[int]) -> np.ndarray:
        raise NotImplementedError


class GaussianNoise(BaseNoise):
    """random.py:23-33: independent N(mu, sigma^2) draws."""

    def __init__(self, mu: float = 0.0, sigma: float = 1.0) -> None:
        super().__init__()
        self._mu = mu
        assert 0 <= sigma, "Noise std should not be negative."
        self._sigma = sigma

    def __call__(self, size: Sequence[int]) -> np.ndarray:
        return np.random.normal(self._mu, self._sigma, size)


class OUNoise(BaseNoise):
    """random.py:36-85: the Ornstein-Uhlenbeck process x += theta dt (mu - x) + sigma sqrt(dt)
    N(0, 1); the state restarts from 0 when the requested shape changes."""

    def __init__(self, mu: float = 0.0, sigma: float = 0.3, theta: float = 0.15,
                 dt: float = 1e-2, x0: Optional[Union[float, np.ndarray]] = None) -> None:
        super().__init__()
        self._mu = mu
        self._alpha = theta * dt
        self._beta = sigma * np.sqrt(dt)
        self._x0 = x0
        self.reset()

    def reset(self) -> None:
        self._x = self._x0

    def __call__(self, size: Sequence[int], mu: Optional[float] = None) -> np.ndarray:
        if self._x is None or isinstance(self._x, np.ndarray) and self._x.shape != size:
            self._x = 0.0
        if mu is None:
            mu = self._mu
        r = self._beta * np.random.normal(size=size)
        self._x = self._x + self._alpha * (mu - self._x) + r
        return self._x
