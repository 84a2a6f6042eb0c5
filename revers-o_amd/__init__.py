"""revers-o embed + search hot path, MI355X-native."""
from .config import PEConfig, VARIANTS, DEFAULT_VARIANT, get_config, available_configs  # noqa: F401
from .config import PETextConfig, TEXT_VARIANTS, get_text_config  # noqa: F401
