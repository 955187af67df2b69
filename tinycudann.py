"""Top-level `tinycudann` name, as imported by PyTorch code written for tiny-cuda-nn's torch modules
(`import tinycudann as tcnn`): the gfx950 autograd modules of neus2_amd.tcnn."""
from neus2_amd.tcnn import Encoding, Module, NativeBackend, Network, NetworkWithInputEncoding  # noqa: F401
