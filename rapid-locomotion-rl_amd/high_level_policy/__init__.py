"""``high_level_policy`` surface of the reference fork: thin re-exports of ``lrl.hlp``."""
from lrl.hlp import HLP_ROOT_DIR, USE_LATENT  # noqa: F401
