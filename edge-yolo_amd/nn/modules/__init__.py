"""Module registry of the detection path (names resolve from YAML `module` strings, like the reference's
`globals()[m]` lookup in nn/tasks.py:984)."""
from .block import (DFL, Proto, SPPF, C2f, C2fAttn, MaxSigmoidAttnBlock, BNContrastiveHead, C3, C3k, C3k2, Bottleneck, Attention, PSABlock, C2PSA, LinearAttention, PSABlock_LinearAttention,
                    C2PSA_LinearAttention, AAttn, ABlock, A2C2f, DSBottleneck, DSC3k, DSC3K2_Wavelet, DSC3K2, AdaHyperedgeGen, AdaHGConv,
                    Mlp, CMlp, LocalAgg, GlobalSparseAttn, SelfAttn, LGLBlock, DSC3K2_LGL,
                    AdaHGComputation, C3AH, FuseModule, HyperACE, DownsampleConv, FullPAD_Tunnel,
                    RepBottleneck, RepCSP, RepNCSPELAN4, ELAN1, SPPELAN, AConv, ADown, CBLinear, CBFuse,
                    SCDown, RepVGGDW, CIB, C2fCIB, PSA, C2, GhostBottleneck, C3Ghost, SPP, ResNetBlock, ResNetLayer)
from .conv import Conv, DWConv, DSConv, RepConv, GhostConv, Concat, Upsample, autopad
from .classic import ConvTranspose2d, MaxPool2d, ZeroPad2d
from .dysample import DySample
from .head import Classify, Detect, E2EDetect, GF2Detect, GFLHeadv2_uniH, OBB, Pose, Segment, WorldDetect, v10Detect

__all__ = ("Conv", "DWConv", "DSConv", "Concat", "Upsample", "autopad", "DFL", "SPPF", "C2f", "C3", "C3k", "C3k2", "Bottleneck", "Attention",
           "PSABlock", "C2PSA", "LinearAttention", "PSABlock_LinearAttention", "C2PSA_LinearAttention", "AAttn", "ABlock", "A2C2f", "DSBottleneck", "DSC3k",
           "DSC3K2_Wavelet", "DSC3K2", "AdaHyperedgeGen", "AdaHGConv", "AdaHGComputation", "C3AH", "FuseModule", "HyperACE", "DownsampleConv",
           "FullPAD_Tunnel", "Mlp", "CMlp", "LocalAgg", "GlobalSparseAttn", "SelfAttn", "LGLBlock", "DSC3K2_LGL", "DySample", "Detect", "Segment", "OBB", "Pose", "Classify", "Proto", "GF2Detect", "E2EDetect", "GFLHeadv2_uniH",
           "C2fAttn", "MaxSigmoidAttnBlock", "BNContrastiveHead", "WorldDetect",
           "RepConv", "RepBottleneck", "RepCSP", "RepNCSPELAN4", "ELAN1", "SPPELAN", "AConv", "ADown", "CBLinear", "CBFuse",
           "SCDown", "RepVGGDW", "CIB", "C2fCIB", "PSA", "v10Detect", "C2", "GhostConv", "GhostBottleneck", "C3Ghost",
           "SPP", "MaxPool2d", "ZeroPad2d", "ConvTranspose2d", "ResNetBlock", "ResNetLayer")
