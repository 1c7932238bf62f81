"""vae_play_amd -- MI355X (gfx950) native back end for the convolutional-VAE training step of
kungyao/vae-play.  Hot path only: drop-in Encoder/Decoder/reparameterize,
HIP kernels behind a C ABI (include/vaeplay_hip.h), flat-arena optimiser, data-parallel step.
Importing the package does not touch the GPU; using any op without libvaeplay_hip.so raises.
"""
from . import _lib  # noqa: F401
from .networks import (VAE, Decoder, DecoderBlock, DirectDecoder, Discriminator, Encoder, EncoderBlock,  # noqa: F401
                       VaeGan, init_parameters, reparameterize)
from .functional import (binary_cross_entropy, get_attention_route, get_conv_precision, kl_divergence,  # noqa: F401
                         set_attention_route, set_conv_precision, vae_loss)
from .infer import FusedVAEInference  # noqa: F401
from .infer_gan import FusedVAEGANInference  # noqa: F401
from .infer_be import FusedBEInference  # noqa: F401
from .be_page import compose_page  # noqa: F401
from .seg_eval import segmentation_metrics, summarize  # noqa: F401
from .infer_font import FusedFontInference  # noqa: F401
from .infer_stylegan import FusedStyleGanInference  # noqa: F401

__all__ = ["VAE", "VaeGan", "Encoder", "Decoder", "Discriminator", "DirectDecoder", "EncoderBlock", "DecoderBlock",
           "reparameterize", "init_parameters",
           "binary_cross_entropy", "kl_divergence", "vae_loss", "set_conv_precision", "get_conv_precision",
           "set_attention_route", "get_attention_route",
           "FusedVAEInference", "FusedVAEGANInference", "FusedBEInference", "FusedFontInference",
           "FusedStyleGanInference", "compose_page", "segmentation_metrics", "summarize"]
