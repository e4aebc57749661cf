from .fourier import FourierNet
from .siren import Siren
from .wavelet_siren import WaveletSiren

# reference: implicit_image/models/__init__.py:5
registry = {"siren": Siren, "fourier": FourierNet, "wavelet_siren": WaveletSiren}
