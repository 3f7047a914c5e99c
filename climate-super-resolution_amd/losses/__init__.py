from .l1 import L1Loss  # noqa: F401
from .mse import MSELoss  # noqa: F401
