"""MuseDiffusion/utils/decode_util.py as a re-export: run/sample.py imports decode_batch, split_meta_midi and
meta_to_batch from here.  meta_to_batch takes the already encoded meta + chord tokens (the meta encoder stays the reference's)."""
from musediffusion_amd.utils.decode_util import (decode_batch, decode_tokens, meta_to_batch, split_meta_midi,  # noqa: F401
                                                 validate_tokens, write_midi)
