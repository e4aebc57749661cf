from .feathernet import FeatherNet

__all__ = ["FeatherNet"]
