"""Speech-to-speech models (``mlx_audio/sts``): speech enhancement.  Models are loaded through ``mlx_audio_amd.sts.loader``."""
