"""Drop-in replacement of the reference's src/MC/trainer.py: `from src.MC.trainer import Trainer` (src/MC/train.py:10) resolves to the
MI355X-native trainer.  Put `dropin/` ahead on sys.path."""
import os
import sys

_root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
if _root not in sys.path:
    sys.path.insert(0, _root)
import cti_amd as _c  # noqa: E402

Trainer = _c.MCTrainer
compute_score_with_logits = _c.compute_score_with_logits
compute_score_mc = _c.compute_score_mc
