"""MI355X-native hot path of yuz1wan/video_distillation (see README.md / DESIGN.md)."""
