"""Device-side batch producers: the reference's data/corruption.py, data/wrapper.py collate and
data/__init__.py load_data_music, running on ragged int32 token tensors that already live on the GPU."""
from .corruption import Corruptions, masking_note, masking_token, random_rotating, randomize_note  # noqa: F401
from .dataset import Augment, MusicDataset, MusicLoader, augment_rows, load_data_music  # noqa: F401
from .wrapper import collate_batches, gather_rows, select_rows, to_ragged  # noqa: F401
