from .fourier import FourierNet
from .siren import Siren

# reference: implicit_image/models/__init__.py:5 (wavelet_siren needs pytorch_wavelets / kornia: outside the hot path)
registry = {"siren": Siren, "fourier": FourierNet}
