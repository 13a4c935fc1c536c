"""Drop-in replacement of the reference's src/FFOE/trainer.py: `from src.FFOE.trainer import Trainer` (src/FFOE/train.py:10) resolves to the
MI355X-native trainer.  Put `dropin/` ahead on sys.path."""
import os
import sys

_root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
if _root not in sys.path:
    sys.path.insert(0, _root)
import cti_amd as _c  # noqa: E402

Trainer = _c.Trainer
compute_score_with_logits = _c.compute_score_with_logits
