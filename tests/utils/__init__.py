from .dist_helpers import (  # noqa: F401
    run_distributed, find_free_port, scratch_dir)
